// PNG encode core, the mirror of png_core.h: colour type, line filter, and a DEFLATE (RFC 1951) writer that cuts the
// filtered rows of an image into independent SEGMENTS.  ONE implementation for the device kernels (png_enc.hip), the
// host entry point gv_png_encode_host and the stand-alone checker (tests/native/png_enc_core_check.cpp): plain g++
// compiles it with the qualifiers defined away, hipcc compiles it for host and device.
//
// Every function is written for a GROUP of lanes (Ctx::lane, Ctx::nlanes, Ctx::sync()): work is dealt to the lanes in
// strides, what has to be serial (the scans over the 256 chunks of a segment, the code lengths, a block's header) is
// done by lane 0 between two sync()s, counters and output words are shared through Ctx::add / Ctx::orr (LDS integer
// atomics on the device, plain += and |= on the host, where the group is one lane).  All of it is integer arithmetic
// whose result does not depend on the order of the adds and ors, so the bytes are the same for any number of lanes.
//
// The stream of an image:   78 01 | segment 0 | segment 1 | ... | Adler-32 of the raw stream, big-endian
// A segment is GV_PNG_ENC_SEG bytes of the raw stream (the last one what is left), encoded on its own as ONE block:
// stored, fixed or dynamic, whichever takes the fewest bits (ties: stored, then fixed).  No match reaches back before
// the segment's first byte.  Every segment but the last is followed by an empty non-final stored block (000, padding
// to the byte, 00 00 FF FF), so a segment starts on a byte boundary and segments concatenate byte-wise; the block of
// the last segment carries BFINAL.
//
// The token rule (one closed form per position i of a segment, D = its bytes, ch = bytes per pixel):
//   class(i) = 1  if i >= 1 and D[i] == D[i-1]                      (a run at distance 1)
//              2  else if ch > 1, i >= ch and D[i] == D[i-ch]       (a run at distance ch)
//              0  otherwise
//   a RUN is a maximal interval [s, e) of positions of one class; it is cut into pieces of 258 positions from s, the
//   last piece is what is left.  A piece of class 1 / 2 and of at least 3 positions is ONE match (its length, distance 1
//   / ch) at its first position; every other position is a literal.
// s and e of a position come from two scans over the run boundaries, so no position waits for the tokens before it.
//
// Bounds: every loop runs over a segment (<= GV_PNG_ENC_SEG), its chunks, or an alphabet; every write into the output
// words is checked against their number; a segment takes at most its size + 10 bytes (the stored form + the marker).
// The functions return a GV_PNG_* status and never trap.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gvcnn_hip.h"
#include "png_core.h"

#define GV_PNG_ENC_SEG 8192                                      // bytes of the raw stream per segment
#define GV_PNG_ENC_CHUNK 32                                      // ... per chunk: the unit a lane walks serially
#define GV_PNG_ENC_NCHUNK (GV_PNG_ENC_SEG / GV_PNG_ENC_CHUNK)
#define GV_PNG_ENC_SEGOUT (GV_PNG_ENC_SEG + 16)                  // bytes of a segment's output slot (>= SEG + 10)
#define GV_PNG_ENC_OUTWORDS (GV_PNG_ENC_SEGOUT / 4)
#define GV_PNG_ENC_NLIT 286
#define GV_PNG_ENC_NDIST 30
#define GV_PNG_ENC_PM (2 * GV_PNG_ENC_NLIT)                      // items of a package-merge list (2 m - 2 are kept)
#define GV_PNG_ENC_META 4                                        // int32 per segment: bytes, Adler a, Adler b, status

// Working set of one segment (the device keeps it in LDS: 47 KB, two workgroups per CU)
struct GvPngEncSeg {
    uint32_t out[GV_PNG_ENC_OUTWORDS];                           // the block's bits, least significant bit first
    uint8_t data[GV_PNG_ENC_SEG];
    uint16_t aux[GV_PNG_ENC_SEG];                                // end of the position's run, then its token: 0 none, 1 literal, 3..258 match
    uint32_t lfreq[288], dfreq[32], cfreq[20];
    uint16_t lcode[288], dcode[32], ccode[20];                   // codes, bit-reversed (the stream takes them MSB first)
    uint8_t llen[288], dlen[32], clen[20];
    uint16_t order[288];                                         // the used symbols of an alphabet by rising frequency
    uint32_t pmw[2][GV_PNG_ENC_PM];                              // package-merge: weights of the previous / current list
    uint32_t pmflag[15][(GV_PNG_ENC_PM + 31) / 32];              // ... per level: item k is a leaf
    uint32_t pmcount[16], cnt[16], next[16];
    uint32_t cfirst[GV_PNG_ENC_NCHUNK], clast[GV_PNG_ENC_NCHUNK];   // run boundaries of a chunk, then the carries into it
    uint32_t cbits[GV_PNG_ENC_NCHUNK], ca[GV_PNG_ENC_NCHUNK], cb[GV_PNG_ENC_NCHUNK];
    uint16_t clseq[320];                                         // the code-length sequence: symbol | extra << 5
    int32_t ncl, hlit, hdist, hclen, choice, overflow;
    uint32_t hdrbits, nbytes, adler_a, adler_b;
};

struct GvPngEncHostCtx {
    int lane = 0, nlanes = 1;
    void sync() const {}
    uint32_t sum(uint32_t v) const { return v; }                 // over the lanes of the group
    void add(uint32_t* p, uint32_t v) const { *p += v; }
    void orr(uint32_t* p, uint32_t v) const { *p |= v; }
};

GV_PNG_HD int64_t gv_png_enc_raw_bytes(int h0, int w0, int ch) { return (int64_t)h0 * (1 + (int64_t)w0 * ch); }
GV_PNG_HD int64_t gv_png_enc_segments(int64_t raw) { return (raw + GV_PNG_ENC_SEG - 1) / GV_PNG_ENC_SEG; }
// most stream bytes of an image: header, every segment stored (5 bytes) and marked (5 bytes), trailer; a multiple of 16
GV_PNG_HD int64_t gv_png_enc_bound(int h0, int w0) {
    const int64_t raw = gv_png_enc_raw_bytes(h0, w0, 3);
    return (2 + raw + 10 * gv_png_enc_segments(raw) + 4 + 15) / 16 * 16;
}

// ---- colour type ----------------------------------------------------------------------------------------------------
// *flag (shared by the group, 0 on entry, read after a sync) becomes 1 when a pixel of src [npix, 3] has R != G or G != B
template <class Ctx>
GV_PNG_HD void gv_png_enc_scan_gray(const uint8_t* src, uint32_t npix, int32_t* flag, const Ctx& ctx) {
    int any = 0;
    for (uint32_t p = (uint32_t)ctx.lane; p < npix; p += (uint32_t)ctx.nlanes) {
        const uint8_t* q = src + (size_t)p * 3;
        any |= (q[0] != q[1]) | (q[1] != q[2]);
    }
    if (any) *flag = 1;                                          // (every writer stores the same value)
}

// ---- line filter ----------------------------------------------------------------------------------------------------
GV_PNG_HD uint32_t gv_png_enc_cost(int v) { return (uint32_t)(v < 128 ? v : 256 - v); }

// byte x of row y of the image as the PNG holds it (ch = 1: the red channel)
GV_PNG_HD int gv_png_enc_px(const uint8_t* src, int w0, int ch, int y, int x) {
    return src[((size_t)y * w0) * 3 + (ch == 1 ? (size_t)x * 3 : (size_t)x)];
}

GV_PNG_HD int gv_png_enc_residual(int ft, int cur, int a, int b, int c) {
    const int p = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : gv_png_paeth(a, b, c);
    return (cur - p) & 255;
}

// Row y of src [h0, w0, 3] -> dst[0] = filter type, dst[1 .. 1 + w0 * ch) = the filtered bytes.  filter: 0-4 forced,
// GV_PNG_FILTER_ADAPTIVE: the type with the smallest sum of |signed residual|, the lowest type on a tie.  Every
// candidate is computed from the UNFILTERED neighbours, so rows are independent.  Returns the type used.
template <class Ctx>
GV_PNG_HD int gv_png_enc_filter_row(const uint8_t* src, int w0, int ch, int y, int filter, uint8_t* dst, const Ctx& ctx) {
    const int rb = w0 * ch;
    int ft = filter;
    if (filter == GV_PNG_FILTER_ADAPTIVE) {
        uint32_t cost[5] = {0, 0, 0, 0, 0};
        for (int x = ctx.lane; x < rb; x += ctx.nlanes) {
            const int cur = gv_png_enc_px(src, w0, ch, y, x), a = x >= ch ? gv_png_enc_px(src, w0, ch, y, x - ch) : 0;
            const int b = y ? gv_png_enc_px(src, w0, ch, y - 1, x) : 0;
            const int c = (y && x >= ch) ? gv_png_enc_px(src, w0, ch, y - 1, x - ch) : 0;
            for (int t = 0; t < 5; ++t) cost[t] += gv_png_enc_cost(gv_png_enc_residual(t, cur, a, b, c));
        }
        uint32_t best = 0;
        ft = 0;
        for (int t = 0; t < 5; ++t) {
            const uint32_t s = ctx.sum(cost[t]);
            if (t == 0 || s < best) {
                best = s;
                ft = t;
            }
        }
    }
    if (ctx.lane == 0) dst[0] = (uint8_t)ft;
    for (int x = ctx.lane; x < rb; x += ctx.nlanes) {
        const int cur = gv_png_enc_px(src, w0, ch, y, x), a = x >= ch ? gv_png_enc_px(src, w0, ch, y, x - ch) : 0;
        const int b = y ? gv_png_enc_px(src, w0, ch, y - 1, x) : 0;
        const int c = (y && x >= ch) ? gv_png_enc_px(src, w0, ch, y - 1, x - ch) : 0;
        dst[1 + x] = (uint8_t)gv_png_enc_residual(ft, cur, a, b, c);
    }
    return ft;
}

// ---- Adler-32 from partial sums ---------------------------------------------------------------------------------------
// (a, b) of the bytes so far, then a piece of `len` bytes whose own sums from (0, 0) are (pa, pb)
GV_PNG_HD void gv_png_enc_adler_append(uint32_t& a, uint32_t& b, uint32_t len, uint32_t pa, uint32_t pb) {
    b = (uint32_t)((b + (uint64_t)(len % 65521u) * a + pb) % 65521u);
    a = (a + pa) % 65521u;
}

// ---- tokens ---------------------------------------------------------------------------------------------------------
GV_PNG_HD int gv_png_enc_class(const uint8_t* d, int i, int ch) {
    if (i >= 1 && d[i] == d[i - 1]) return 1;
    if (ch > 1 && i >= ch && d[i] == d[i - ch]) return 2;
    return 0;
}
// a run starts at i
GV_PNG_HD bool gv_png_enc_boundary(const uint8_t* d, int i, int ch) {
    return i == 0 || gv_png_enc_class(d, i, ch) != gv_png_enc_class(d, i - 1, ch);
}

// length 3..258 -> its symbol, the number of extra bits and their value
GV_PNG_HD void gv_png_enc_lensym(int len, int& sym, int& eb, int& extra) {
    const int l = len - 3;
    sym = 285;
    eb = 0;
    extra = 0;
    if (len >= 258) return;
    if (l < 8) {
        sym = 257 + l;
        return;
    }
    eb = 29 - __builtin_clz((unsigned)l);                        // floor(log2 l) - 2
    sym = 261 + 4 * eb + ((l >> eb) & 3);
    extra = l & ((1 << eb) - 1);
}
GV_PNG_HD int gv_png_enc_len_extra_bits(int sym) { return (sym < 265 || sym >= 285) ? 0 : (sym - 261) >> 2; }
GV_PNG_HD int gv_png_enc_fixed_len(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }

// v (nbits <= 32 of it, the rest 0) into the output words at bit `pos`
template <class Ctx>
GV_PNG_HD void gv_png_enc_put(GvPngEncSeg* S, uint32_t pos, uint32_t v, int nbits, const Ctx& ctx) {
    if (nbits <= 0) return;
    const uint32_t w = pos >> 5;
    const uint64_t x = (uint64_t)v << (pos & 31);
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    if (w >= GV_PNG_ENC_OUTWORDS || ((pos & 31) + (uint32_t)nbits > 32 && w + 1 >= GV_PNG_ENC_OUTWORDS)) {
        S->overflow = 1;
        return;
    }
    if (lo) ctx.orr(&S->out[w], lo);
    if (hi) ctx.orr(&S->out[w + 1], hi);
}

// ---- code lengths: package-merge (optimal under a length limit) ---------------------------------------------------
// lane 0: lens[] of the m used symbols S->order[0, m) (rising frequency) of freq[0, n), no code longer than `limit`
// (2^limit >= m).  List `lv` (0 = the deepest level) is the leaves merged with the pairs of list lv - 1, a leaf first on
// a tie, cut to 2 m - 2 items; only "item k is a leaf" is kept per level.  The top list's first 2 m - 2 items are the
// solution: the c leaves among them are the c rarest symbols, each one bit deeper; its k - c packages are the first
// 2 (k - c) items of the list below, and so on down.
GV_PNG_HD void gv_png_enc_package_merge(const uint32_t* freq, int n, int limit, uint8_t* lens, GvPngEncSeg* S) {
    int m = 0;
    for (int s = 0; s < n; ++s) m += freq[s] != 0;
    if (m == 0) return;
    if (m == 1) {
        lens[S->order[0]] = 1;
        return;
    }
    const int keep = 2 * m - 2;
    int plen = 0, pv = 0;
    for (int lv = 0; lv < limit; ++lv) {
        const uint32_t* prev = S->pmw[pv];
        uint32_t* cur = S->pmw[pv ^ 1];
        const int np = plen >> 1;
        int li = 0, pi = 0, k = 0;
        uint32_t word = 0;
        while (k < keep && (li < m || pi < np)) {
            const uint32_t pw = pi < np ? prev[2 * pi] + prev[2 * pi + 1] : 0u;
            const uint32_t lw = li < m ? freq[S->order[li]] : 0u;
            const bool leaf = li < m && (pi >= np || lw <= pw);
            cur[k] = leaf ? lw : pw;
            if (leaf) {
                ++li;
                word |= 1u << (k & 31);
            } else {
                ++pi;
            }
            ++k;
            if ((k & 31) == 0) {
                S->pmflag[lv][(k >> 5) - 1] = word;
                word = 0;
            }
        }
        if (k & 31) S->pmflag[lv][k >> 5] = word;
        plen = k;
        pv ^= 1;
    }
    for (int lv = 0; lv < 16; ++lv) S->pmcount[lv] = 0;
    int k = keep < plen ? keep : plen;
    for (int lv = limit - 1; lv >= 0 && k > 0; --lv) {
        int c = 0;
        for (int w = 0; w < (k >> 5); ++w) c += __builtin_popcount(S->pmflag[lv][w]);
        if (k & 31) c += __builtin_popcount(S->pmflag[lv][k >> 5] & ((1u << (k & 31)) - 1u));
        S->pmcount[lv] = (uint32_t)c;
        k = 2 * (k - c);
    }
    for (int idx = 0; idx < m; ++idx) {
        int l = 0;
        for (int lv = 0; lv < limit; ++lv) l += S->pmcount[lv] > (uint32_t)idx;
        lens[S->order[idx]] = (uint8_t)l;
    }
}

// the group: lens[0, n) from freq[0, n) — the lanes rank the used symbols, lane 0 runs the package-merge
template <class Ctx>
GV_PNG_HD void gv_png_enc_lengths(const uint32_t* freq, int n, int limit, uint8_t* lens, GvPngEncSeg* S, const Ctx& ctx) {
    ctx.sync();
    for (int s = ctx.lane; s < n; s += ctx.nlanes) {
        const uint32_t f = freq[s];
        lens[s] = 0;
        if (!f) continue;
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t g = freq[j];
            rank += (g && (g < f || (g == f && j < s))) ? 1 : 0;
        }
        S->order[rank] = (uint16_t)s;
    }
    ctx.sync();
    if (ctx.lane == 0) gv_png_enc_package_merge(freq, n, limit, lens, S);
    ctx.sync();
}

// lane 0: canonical codes of lens[0, n), bit-reversed
GV_PNG_HD void gv_png_enc_codes(const uint8_t* lens, int n, uint16_t* code, GvPngEncSeg* S) {
    for (int l = 0; l < 16; ++l) S->cnt[l] = 0;
    for (int i = 0; i < n; ++i) S->cnt[lens[i] & 15]++;
    S->cnt[0] = 0;
    uint32_t c = 0;
    S->next[0] = 0;
    for (int l = 1; l < 16; ++l) {
        c = (c + S->cnt[l - 1]) << 1;
        S->next[l] = c;
    }
    for (int i = 0; i < n; ++i) {
        const int l = lens[i] & 15;
        code[i] = 0;
        if (!l) continue;
        uint32_t v = S->next[l]++, rev = 0;
        for (int j = 0; j < l; ++j) {
            rev = (rev << 1) | (v & 1);
            v >>= 1;
        }
        code[i] = (uint16_t)rev;
    }
}

GV_PNG_HD int gv_png_enc_cl_value(const GvPngEncSeg* S, int i) { return i < S->hlit ? S->llen[i] : S->dlen[i - S->hlit]; }
GV_PNG_HD void gv_png_enc_cl_emit(GvPngEncSeg* S, int sym, int extra) {
    if (S->ncl < 320) S->clseq[S->ncl++] = (uint16_t)(sym | extra << 5);
    else S->overflow = 1;
    S->cfreq[sym]++;
}
// lane 0: hlit, hdist and the run-length form of the two length tables (symbols 16 / 17 / 18), with its histogram
GV_PNG_HD void gv_png_enc_cl_sequence(GvPngEncSeg* S) {
    int hlit = GV_PNG_ENC_NLIT, hdist = GV_PNG_ENC_NDIST;
    while (hlit > 257 && S->llen[hlit - 1] == 0) --hlit;
    while (hdist > 1 && S->dlen[hdist - 1] == 0) --hdist;
    S->hlit = hlit;
    S->hdist = hdist;
    S->ncl = 0;
    const int total = hlit + hdist;
    int i = 0;
    while (i < total) {
        const int v = gv_png_enc_cl_value(S, i);
        int run = 1;
        while (i + run < total && gv_png_enc_cl_value(S, i + run) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int r = run < 138 ? run : 138;
                gv_png_enc_cl_emit(S, 18, r - 11);
                run -= r;
            }
            if (run >= 3) {
                gv_png_enc_cl_emit(S, 17, run - 3);
                run = 0;
            }
            for (; run > 0; --run) gv_png_enc_cl_emit(S, 0, 0);
        } else {
            gv_png_enc_cl_emit(S, v, 0);
            --run;
            while (run >= 3) {
                const int r = run < 6 ? run : 6;
                gv_png_enc_cl_emit(S, 16, r - 3);
                run -= r;
            }
            for (; run > 0; --run) gv_png_enc_cl_emit(S, v, 0);
        }
    }
}

// lane 0: the three costs, the choice (0 stored, 1 fixed, 2 dynamic), the tables of the choice and the block's header
template <class Ctx>
GV_PNG_HD void gv_png_enc_choose(GvPngEncSeg* S, uint32_t n, int last, const Ctx& ctx) {
    uint32_t extra = 0, dyn = 0, fix = 0;
    int used = 0, only = 0;
    for (int s = 0; s < 19; ++s)
        if (S->clen[s]) {
            ++used;
            only = s;
        }
    if (used == 1) S->clen[only ? 0 : 1] = 1;                    // (a code-length code must be complete: a second 1-bit code)
    for (int s = 0; s < GV_PNG_ENC_NLIT; ++s) {
        const uint32_t f = S->lfreq[s];
        extra += f * (uint32_t)gv_png_enc_len_extra_bits(s);
        dyn += f * S->llen[s];
        fix += f * (uint32_t)gv_png_enc_fixed_len(s);
    }
    for (int s = 0; s < GV_PNG_ENC_NDIST; ++s) {                 // (distances 1 and ch <= 4 have no extra bits)
        dyn += S->dfreq[s] * S->dlen[s];
        fix += S->dfreq[s] * 5u;
    }
    int hclen = 19;
    while (hclen > 4 && S->clen[gv_png_clen_order(hclen - 1)] == 0) --hclen;
    S->hclen = hclen;
    uint32_t hdr = 3 + 14 + 3 * (uint32_t)hclen;
    for (int k = 0; k < S->ncl; ++k) {
        const int sym = S->clseq[k] & 31;
        hdr += S->clen[sym] + (sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u);
    }
    dyn += hdr + extra;
    fix += 3 + extra;
    const uint32_t stored = 8u * (5u + n);
    const int choice = (stored <= fix && stored <= dyn) ? 0 : fix <= dyn ? 1 : 2;
    S->choice = choice;
    gv_png_enc_put(S, 0, (uint32_t)(last ? 1 : 0), 1, ctx);
    if (choice == 0) {
        gv_png_enc_put(S, 8, n & 0xffffu, 16, ctx);
        gv_png_enc_put(S, 24, ~n & 0xffffu, 16, ctx);
        S->hdrbits = 40;
        return;
    }
    gv_png_enc_put(S, 1, (uint32_t)choice, 2, ctx);
    if (choice == 1) {
        for (int s = 0; s < 288; ++s) S->llen[s] = (uint8_t)gv_png_enc_fixed_len(s);
        for (int s = 0; s < 32; ++s) S->dlen[s] = 5;
        gv_png_enc_codes(S->llen, 288, S->lcode, S);
        gv_png_enc_codes(S->dlen, 32, S->dcode, S);
        S->hdrbits = 3;
        return;
    }
    gv_png_enc_codes(S->llen, GV_PNG_ENC_NLIT, S->lcode, S);
    gv_png_enc_codes(S->dlen, GV_PNG_ENC_NDIST, S->dcode, S);
    gv_png_enc_codes(S->clen, 19, S->ccode, S);
    uint32_t pos = 3;
    gv_png_enc_put(S, pos, (uint32_t)(S->hlit - 257), 5, ctx);
    gv_png_enc_put(S, pos + 5, (uint32_t)(S->hdist - 1), 5, ctx);
    gv_png_enc_put(S, pos + 10, (uint32_t)(hclen - 4), 4, ctx);
    pos += 14;
    for (int k = 0; k < hclen; ++k, pos += 3) gv_png_enc_put(S, pos, S->clen[gv_png_clen_order(k)], 3, ctx);
    for (int k = 0; k < S->ncl; ++k) {
        const int sym = S->clseq[k] & 31, ex = S->clseq[k] >> 5;
        gv_png_enc_put(S, pos, S->ccode[sym], S->clen[sym], ctx);
        pos += S->clen[sym];
        const int eb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
        gv_png_enc_put(S, pos, (uint32_t)ex, eb, ctx);
        pos += (uint32_t)eb;
    }
    S->hdrbits = pos;
}

// One segment: src[0, n) (n <= GV_PNG_ENC_SEG bytes of the raw stream, src 4-byte aligned) -> dst (a slot of
// GV_PNG_ENC_SEGOUT bytes, 4-byte aligned) and meta[0, 4) = bytes written, the segment's Adler sums (a, b) from (0, 0),
// status.  ch: bytes per pixel; last: the block carries BFINAL and no marker follows.
template <class Ctx>
GV_PNG_HD int gv_png_enc_segment(const uint8_t* src, uint32_t n, int ch, int last, GvPngEncSeg* S, uint8_t* dst,
                                 int32_t* meta, const Ctx& ctx) {
    if (n == 0 || n > GV_PNG_ENC_SEG) {
        if (ctx.lane == 0) {
            meta[0] = 0;
            meta[1] = 0;
            meta[2] = 0;
            meta[3] = GV_PNG_TOO_LONG;
        }
        return GV_PNG_TOO_LONG;
    }
    const int lane = ctx.lane, nl = ctx.nlanes, N = (int)n;
    const int nchunk = (N + GV_PNG_ENC_CHUNK - 1) / GV_PNG_ENC_CHUNK;
    ctx.sync();                                                  // (the previous segment's readers are done)
    for (int i = lane; i < GV_PNG_ENC_OUTWORDS; i += nl) S->out[i] = 0;
    for (int i = lane; i < 288; i += nl) S->lfreq[i] = 0;
    for (int i = lane; i < 32; i += nl) S->dfreq[i] = 0;
    for (int i = lane; i < 20; i += nl) {
        S->cfreq[i] = 0;
        S->clen[i] = 0;
    }
    if (lane == 0) S->overflow = 0;
    for (int i = lane * 4; i < N; i += nl * 4) {
        if (i + 4 <= N) {
            const uint32_t v = gv_png_load32(src + i);
            __builtin_memcpy(S->data + i, &v, 4);
        } else {
            for (int k = i; k < N; ++k) S->data[k] = src[k];
        }
    }
    ctx.sync();
    const uint8_t* D = S->data;
    // the run boundaries of every chunk: its first and its last
    for (int c = lane; c < nchunk; c += nl) {
        const int lo = c * GV_PNG_ENC_CHUNK, hi = lo + GV_PNG_ENC_CHUNK < N ? lo + GV_PNG_ENC_CHUNK : N;
        uint32_t first = 0xffffffffu, lastb = 0xffffffffu;
        for (int i = lo; i < hi; ++i)
            if (gv_png_enc_boundary(D, i, ch)) {
                if (first == 0xffffffffu) first = (uint32_t)i;
                lastb = (uint32_t)i;
            }
        S->cfirst[c] = first;
        S->clast[c] = lastb;
    }
    ctx.sync();
    if (lane == 0) {                                             // -> the carries: the last boundary before a chunk, the first behind it
        uint32_t s = 0;
        for (int c = 0; c < nchunk; ++c) {
            const uint32_t mine = S->clast[c];
            S->clast[c] = s;
            if (mine != 0xffffffffu) s = mine;
        }
        uint32_t e = n;
        for (int c = nchunk - 1; c >= 0; --c) {
            const uint32_t mine = S->cfirst[c];
            S->cfirst[c] = e;
            if (mine != 0xffffffffu) e = mine;
        }
    }
    ctx.sync();
    // the token of every position, the histograms, the Adler sums of the chunk
    for (int c = lane; c < nchunk; c += nl) {
        const int lo = c * GV_PNG_ENC_CHUNK, hi = lo + GV_PNG_ENC_CHUNK < N ? lo + GV_PNG_ENC_CHUNK : N;
        uint32_t e = S->cfirst[c];
        for (int i = hi - 1; i >= lo; --i) {
            S->aux[i] = (uint16_t)e;                             // (e <= 8192 fits)
            if (gv_png_enc_boundary(D, i, ch)) e = (uint32_t)i;
        }
        uint32_t s = S->clast[c], a = 0, b = 0;
        for (int i = lo; i < hi; ++i) {
            if (gv_png_enc_boundary(D, i, ch)) s = (uint32_t)i;
            const int cl = gv_png_enc_class(D, i, ch);
            int tok = 1;
            if (cl) {
                const int o = i - (int)s, cs = i - o % 258;
                const int len = (int)S->aux[i] - cs < 258 ? (int)S->aux[i] - cs : 258;
                if (len >= 3) tok = i == cs ? len : 0;
            }
            S->aux[i] = (uint16_t)tok;
            if (tok == 1) {
                ctx.add(&S->lfreq[D[i]], 1u);
            } else if (tok) {
                int sym, eb, ex;
                gv_png_enc_lensym(tok, sym, eb, ex);
                ctx.add(&S->lfreq[sym], 1u);
                ctx.add(&S->dfreq[cl == 1 ? 0 : ch - 1], 1u);
            }
            a += D[i];
            b += a;
        }
        S->ca[c] = a;
        S->cb[c] = b;
    }
    ctx.sync();
    if (lane == 0) {
        S->lfreq[256] = 1;                                       // the end-of-block symbol
        uint32_t a = 0, b = 0;
        for (int c = 0; c < nchunk; ++c) {
            const int lo = c * GV_PNG_ENC_CHUNK, hi = lo + GV_PNG_ENC_CHUNK < N ? lo + GV_PNG_ENC_CHUNK : N;
            gv_png_enc_adler_append(a, b, (uint32_t)(hi - lo), S->ca[c], S->cb[c]);
        }
        S->adler_a = a;
        S->adler_b = b;
    }
    gv_png_enc_lengths(S->lfreq, GV_PNG_ENC_NLIT, 15, S->llen, S, ctx);
    gv_png_enc_lengths(S->dfreq, GV_PNG_ENC_NDIST, 15, S->dlen, S, ctx);
    if (lane == 0) gv_png_enc_cl_sequence(S);
    gv_png_enc_lengths(S->cfreq, 19, 7, S->clen, S, ctx);
    if (lane == 0) gv_png_enc_choose(S, n, last, ctx);
    ctx.sync();
    const int choice = S->choice;
    // bits of every chunk's tokens, then where each chunk starts
    if (choice) {
        for (int c = lane; c < nchunk; c += nl) {
            const int lo = c * GV_PNG_ENC_CHUNK, hi = lo + GV_PNG_ENC_CHUNK < N ? lo + GV_PNG_ENC_CHUNK : N;
            uint32_t bits = 0;
            for (int i = lo; i < hi; ++i) {
                const int tok = S->aux[i];
                if (tok == 1) {
                    bits += S->llen[D[i]];
                } else if (tok) {
                    int sym, eb, ex;
                    gv_png_enc_lensym(tok, sym, eb, ex);
                    bits += S->llen[sym] + (uint32_t)eb + S->dlen[gv_png_enc_class(D, i, ch) == 1 ? 0 : ch - 1];
                }
            }
            S->cbits[c] = bits;
        }
    }
    ctx.sync();
    if (lane == 0) {
        uint32_t pos = S->hdrbits;
        if (choice) {
            for (int c = 0; c < nchunk; ++c) {
                const uint32_t mine = S->cbits[c];
                S->cbits[c] = pos;
                pos += mine;
            }
            gv_png_enc_put(S, pos, S->lcode[256], S->llen[256], ctx);
            pos += S->llen[256];
        } else {
            pos += 8u * n;
        }
        if (last) {
            S->nbytes = (pos + 7) >> 3;
        } else {                                                 // 000, to the byte, LEN = 0, NLEN = ffff
            const uint32_t pb = (pos + 3 + 7) >> 3;
            gv_png_enc_put(S, 8 * (pb + 2), 0xffffu, 16, ctx);
            S->nbytes = pb + 4;
        }
    }
    ctx.sync();
    for (int c = lane; c < nchunk; c += nl) {
        const int lo = c * GV_PNG_ENC_CHUNK, hi = lo + GV_PNG_ENC_CHUNK < N ? lo + GV_PNG_ENC_CHUNK : N;
        if (!choice) {
            for (int i = lo; i < hi; i += 4) {
                const int k = hi - i < 4 ? hi - i : 4;
                uint32_t v = 0;
                for (int j = 0; j < k; ++j) v |= (uint32_t)D[i + j] << (8 * j);
                gv_png_enc_put(S, 40u + 8u * (uint32_t)i, v, 8 * k, ctx);
            }
            continue;
        }
        uint32_t pos = S->cbits[c];
        for (int i = lo; i < hi; ++i) {
            const int tok = S->aux[i];
            if (tok == 1) {
                gv_png_enc_put(S, pos, S->lcode[D[i]], S->llen[D[i]], ctx);
                pos += S->llen[D[i]];
            } else if (tok) {
                int sym, eb, ex;
                gv_png_enc_lensym(tok, sym, eb, ex);
                const int ds = gv_png_enc_class(D, i, ch) == 1 ? 0 : ch - 1;
                gv_png_enc_put(S, pos, (uint32_t)S->lcode[sym] | (uint32_t)ex << S->llen[sym], S->llen[sym] + eb, ctx);
                pos += S->llen[sym] + (uint32_t)eb;
                gv_png_enc_put(S, pos, S->dcode[ds], S->dlen[ds], ctx);
                pos += S->dlen[ds];
            }
        }
    }
    ctx.sync();
    const uint32_t nbytes = S->nbytes;
    const int st = (S->overflow || nbytes > GV_PNG_ENC_SEGOUT) ? GV_PNG_TOO_LONG : GV_PNG_OK;
    const uint32_t nw = st == GV_PNG_OK ? (nbytes + 3) >> 2 : 0;
    for (uint32_t w = (uint32_t)lane; w < nw; w += (uint32_t)nl) __builtin_memcpy(dst + 4 * (size_t)w, &S->out[w], 4);
    if (lane == 0) {
        meta[0] = st == GV_PNG_OK ? (int32_t)nbytes : 0;
        meta[1] = (int32_t)S->adler_a;
        meta[2] = (int32_t)S->adler_b;
        meta[3] = st;
    }
    return st;
}

// The serial encoder of the host twin: one image src [h0, w0, 3] -> its zlib stream in dst[0, *length) (cap bytes, at
// least gv_png_enc_bound(h0, w0)) and *color_type.  rows: h0 * (1 + 3 * w0) bytes, 4-byte aligned; slot:
// GV_PNG_ENC_SEGOUT bytes, 4-byte aligned; seg: working set.  GV_PNG_OK, or GV_PNG_TOO_LONG when a segment or `cap` is
// exceeded (neither happens with cap >= the bound).
inline int gv_png_enc_image_serial(const uint8_t* src, int h0, int w0, int filter, int color, uint8_t* rows, uint8_t* slot,
                                   GvPngEncSeg* seg, uint8_t* dst, int64_t cap, int32_t* length, int32_t* color_type) {
    const GvPngEncHostCtx ctx;
    int32_t flag = 0;
    if (color == GV_PNG_COLOR_AUTO) gv_png_enc_scan_gray(src, (uint32_t)h0 * (uint32_t)w0, &flag, ctx);
    const int ch = (color != GV_PNG_COLOR_AUTO || flag) ? 3 : 1;
    *color_type = ch == 1 ? 0 : 2;
    for (int y = 0; y < h0; ++y) gv_png_enc_filter_row(src, w0, ch, y, filter, rows + (size_t)y * (1 + (size_t)w0 * ch), ctx);
    const int64_t raw = gv_png_enc_raw_bytes(h0, w0, ch), segs = gv_png_enc_segments(raw);
    if (cap < 6) return GV_PNG_TOO_LONG;
    int64_t pos = 2;
    uint32_t a = 1, b = 0;
    dst[0] = 0x78;
    dst[1] = 0x01;
    for (int64_t s = 0; s < segs; ++s) {
        const int64_t off = s * GV_PNG_ENC_SEG;
        const uint32_t len = (uint32_t)(raw - off < GV_PNG_ENC_SEG ? raw - off : GV_PNG_ENC_SEG);
        int32_t meta[GV_PNG_ENC_META];
        const int st = gv_png_enc_segment(rows + off, len, ch, s == segs - 1, seg, slot, meta, ctx);
        if (st != GV_PNG_OK) return st;
        if (pos + meta[0] + 4 > cap) return GV_PNG_TOO_LONG;
        __builtin_memcpy(dst + pos, slot, (size_t)meta[0]);
        pos += meta[0];
        gv_png_enc_adler_append(a, b, len, (uint32_t)meta[1], (uint32_t)meta[2]);
    }
    dst[pos] = (uint8_t)(b >> 8);
    dst[pos + 1] = (uint8_t)b;
    dst[pos + 2] = (uint8_t)(a >> 8);
    dst[pos + 3] = (uint8_t)a;
    *length = (int32_t)(pos + 4);
    return GV_PNG_OK;
}
