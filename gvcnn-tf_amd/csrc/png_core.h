// PNG decode core: DEFLATE (RFC 1951) inside a zlib wrapper (RFC 1950), and the serial un-filter + expand of the host
// twin.  ONE implementation for the device kernel (png.hip), the host entry point gv_png_decode_host and the
// stand-alone checker (tests/native/png_core_check.cpp): plain g++ / clang++ compile it with the qualifiers defined
// away, hipcc compiles it for host and device.
//
// The decoder is written for a GROUP of lanes that all run it on the same stream (Ctx::nlanes, Ctx::lane, Ctx::sync()):
// every lane keeps the same bit-reader state and takes the same branches (what is loaded from memory passes through
// Ctx::uni(), which on the device tells the compiler so: the decode then runs on the scalar unit), the code tables live
// in ONE GvPngTables that lane 0 builds, lane 0 stores literals, and the lanes share the bytes of a match / a stored block / the checksum.
// On the host the group is one lane and sync() does nothing.  Where the output lives is the context's business too
// (put / get / wrote / finish): the host writes `out` directly; the device kernel keeps the last 64 KB in an LDS ring —
// the DEFLATE window, so a match never waits for global memory — and flushes completed pieces to `out`.
//
// Bounds: the output size is known up front (IHDR: h * (1 + w * ch)); every output write is checked against it, every
// input read against the stream length, every match distance against the bytes produced so far.  Every loop iteration
// consumes input bits or emits output, so the decoder ends on any input; it returns a GV_PNG_* status, never traps.
#pragma once
#include <stdint.h>

#include "gvcnn_hip.h"

#if defined(__HIPCC__)
#define GV_PNG_HD __host__ __device__ inline
#else
#define GV_PNG_HD inline
#endif

#define GV_PNG_LFAST 10                                          // bits of the one-step literal/length table
#define GV_PNG_DFAST 8                                           // ... of the distance table
#define GV_PNG_CFAST 7                                           // ... of the code-length table (its codes are <= 7 bits)

// Decode tables of one block.  fast[]: indexed by the next FAST bits of the stream, (symbol << 4) | code length, 0 = a
// longer (or unused) code: those go through count[] / sym[] (canonical order) one bit at a time.
struct GvPngTables {
    uint16_t lfast[1 << GV_PNG_LFAST], dfast[1 << GV_PNG_DFAST], cfast[1 << GV_PNG_CFAST];
    uint16_t lsym[288], dsym[32], csym[20];
    uint16_t lcount[16], dcount[16], ccount[16];
    uint16_t offs[16];
    uint8_t lens[320];
    uint32_t red[128];                                           // per-lane Adler-32 partials (nlanes <= 64)
    int32_t status;
};

struct GvPngHuff {
    uint16_t* fast;
    uint16_t* sym;
    uint16_t* count;
    int fastbits;
};

struct GvPngBits {
    const uint8_t* in;
    uint32_t len, pos;                                           // pos: the first byte not yet in buf (pos <= len)
    uint64_t buf;
    int cnt;
    uint32_t ahead;                                              // in[pos, pos + 4) when len - pos >= 4
};

struct GvPngHostCtx {
    int lane = 0, nlanes = 1;
    void sync() const {}
    uint32_t uni(uint32_t v) const { return v; }                 // a value every lane holds: lets the device keep it scalar
    void put(uint8_t* out, uint32_t pos, uint8_t v) const { out[pos] = v; }
    uint8_t get(const uint8_t* out, uint32_t pos) const { return out[pos]; }
    void wrote(uint8_t*, uint32_t, uint32_t) const {}            // output [from, to) is complete (to - from <= max_run)
    void finish(uint8_t*, uint32_t) const {}                     // the whole output [0, op) must now be in `out`
    uint32_t max_run() const { return 65535u; }
};

GV_PNG_HD int gv_png_channels(int ctype) {
    return ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
}

GV_PNG_HD uint32_t gv_png_load32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);                                  // (little-endian hosts and the GPU alike)
    return v;
}

// (re)start reading at byte `pos`: the next four bytes are fetched AHEAD of their use, so that the load's latency passes
// while the bits in hand are decoded
template <class Ctx>
GV_PNG_HD void gv_png_seek(GvPngBits& b, uint32_t pos, const Ctx& ctx) {
    b.pos = pos;
    b.buf = 0;
    b.cnt = 0;
    b.ahead = b.len - pos >= 4 ? ctx.uni(gv_png_load32(b.in + pos)) : 0;
}

// at least 32 valid bits afterwards unless the stream ends first (missing bits read as 0, cnt says how many are real)
template <class Ctx>
GV_PNG_HD void gv_png_refill(GvPngBits& b, const Ctx& ctx) {
    if (b.cnt > 32) return;
    if (b.len - b.pos >= 4) {
        b.buf |= (uint64_t)b.ahead << b.cnt;
        b.pos += 4;
        b.cnt += 32;
        if (b.len - b.pos >= 4) b.ahead = ctx.uni(gv_png_load32(b.in + b.pos));
    } else {
        while (b.cnt <= 56 && b.pos < b.len) {                   // the last three bytes of a stream at most
            b.buf |= (uint64_t)ctx.uni(b.in[b.pos++]) << b.cnt;
            b.cnt += 8;
        }
    }
}

// n <= 16 bits, or -1 when the stream has fewer left
template <class Ctx>
GV_PNG_HD int gv_png_bits(GvPngBits& b, int n, const Ctx& ctx) {
    gv_png_refill(b, ctx);
    if (b.cnt < n) return -1;
    const int v = (int)(b.buf & ((1u << n) - 1));
    b.buf >>= n;
    b.cnt -= n;
    return v;
}

// kind: 0 code lengths, 1 literal/length, 2 distance.  zlib's rules (inftrees.c): an over-subscribed set is an error; an
// incomplete one too, except a literal/length or distance set whose only code has length 1; no code at all builds an
// empty table (every symbol decoded from it is an error).
GV_PNG_HD int gv_png_build(const GvPngHuff& h, const uint8_t* lens, int n, int kind, uint16_t* offs) {
    for (int l = 0; l < 16; ++l) h.count[l] = 0;
    for (int i = 0; i < n; ++i) h.count[lens[i] & 15]++;
    for (int i = 0; i < (1 << h.fastbits); ++i) h.fast[i] = 0;
    int max = 15;
    while (max > 0 && h.count[max] == 0) --max;
    h.count[0] = 0;
    if (max == 0) return GV_PNG_OK;
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left = left * 2 - (int)h.count[l];
        if (left < 0) return GV_PNG_BAD_CODES;
    }
    if (left > 0 && (kind == 0 || max != 1)) return GV_PNG_BAD_CODES;
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
    for (int i = 0; i < n; ++i)
        if (lens[i] & 15) h.sym[offs[lens[i] & 15]++] = (uint16_t)i;
    int code = 0, idx = 0;
    for (int l = 1; l <= h.fastbits; ++l) {
        code <<= 1;
        for (int k = 0; k < (int)h.count[l]; ++k) {
            int c = code + k, rev = 0;
            for (int j = 0; j < l; ++j) {                        // the stream carries a code most significant bit first
                rev = (rev << 1) | (c & 1);
                c >>= 1;
            }
            const uint16_t e = (uint16_t)((h.sym[idx + k] << 4) | l);
            for (int j = rev; j < (1 << h.fastbits); j += 1 << l) h.fast[j] = e;
        }
        code += h.count[l];
        idx += h.count[l];
    }
    return GV_PNG_OK;
}

// the next symbol (>= 0), or -status
template <class Ctx>
GV_PNG_HD int gv_png_symbol(GvPngBits& b, const GvPngHuff& h, const Ctx& ctx) {
    gv_png_refill(b, ctx);
    const uint32_t e = ctx.uni(h.fast[b.buf & ((1u << h.fastbits) - 1)]);
    if (e) {
        const int l = e & 15;
        if (l > b.cnt) return -GV_PNG_TRUNCATED;
        b.buf >>= l;
        b.cnt -= l;
        return e >> 4;
    }
    int code = 0, first = 0, idx = 0;
    for (int l = 1; l < 16; ++l) {
        if (l > b.cnt) return -GV_PNG_TRUNCATED;
        code |= (int)((b.buf >> (l - 1)) & 1);
        const int cnt = (int)ctx.uni(h.count[l]);
        if (code - first < cnt) {
            b.buf >>= l;
            b.cnt -= l;
            return (int)ctx.uni(h.sym[idx + (code - first)]);
        }
        idx += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return -GV_PNG_BAD_CODES;
}

// order in which a dynamic block sends the lengths of its code-length code: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
GV_PNG_HD int gv_png_clen_order(int i) {
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                        10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}

// tables of a fixed (type 1) or dynamic (type 2) block; every lane reads the header bits, lane 0 writes the tables
template <class Ctx>
GV_PNG_HD int gv_png_block_tables(GvPngBits& b, int type, GvPngTables* t, const Ctx& ctx) {
    const GvPngHuff lit = {t->lfast, t->lsym, t->lcount, GV_PNG_LFAST};
    const GvPngHuff dst = {t->dfast, t->dsym, t->dcount, GV_PNG_DFAST};
    const GvPngHuff cl = {t->cfast, t->csym, t->ccount, GV_PNG_CFAST};
    ctx.sync();                                                  // nobody still reads the previous block's tables
    int hlit = 288, hdist = 32;
    if (type == 1) {
        if (ctx.lane == 0) {
            for (int i = 0; i < 288; ++i) t->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
            for (int i = 0; i < 32; ++i) t->lens[288 + i] = 5;
        }
    } else {
        hlit = gv_png_bits(b, 5, ctx);
        hdist = gv_png_bits(b, 5, ctx);
        const int hclen = gv_png_bits(b, 4, ctx);
        if (hlit < 0 || hdist < 0 || hclen < 0) return GV_PNG_TRUNCATED;
        hlit += 257;
        hdist += 1;
        if (hlit > 286 || hdist > 30) return GV_PNG_BAD_CODES;
        if (ctx.lane == 0)
            for (int i = 0; i < 19; ++i) t->lens[i] = 0;
        for (int i = 0; i < hclen + 4; ++i) {
            const int v = gv_png_bits(b, 3, ctx);
            if (v < 0) return GV_PNG_TRUNCATED;
            if (ctx.lane == 0) t->lens[gv_png_clen_order(i)] = (uint8_t)v;
        }
        if (ctx.lane == 0) t->status = gv_png_build(cl, t->lens, 19, 0, t->offs);
        ctx.sync();
        if (ctx.uni((uint32_t)t->status) != GV_PNG_OK) return (int)ctx.uni((uint32_t)t->status);
        int i = 0, prev = 0;
        while (i < hlit + hdist) {                               // (every pass consumes at least one bit or returns)
            const int s = gv_png_symbol(b, cl, ctx);
            if (s < 0) return -s;
            int rep = 1, val = s;
            if (s == 16) {
                if (i == 0) return GV_PNG_BAD_CODES;
                rep = gv_png_bits(b, 2, ctx) + 3;
                val = prev;
                if (rep < 3) return GV_PNG_TRUNCATED;
            } else if (s == 17) {
                rep = gv_png_bits(b, 3, ctx) + 3;
                val = 0;
                if (rep < 3) return GV_PNG_TRUNCATED;
            } else if (s == 18) {
                rep = gv_png_bits(b, 7, ctx) + 11;
                val = 0;
                if (rep < 11) return GV_PNG_TRUNCATED;
            }
            if (i + rep > hlit + hdist) return GV_PNG_BAD_CODES;
            if (ctx.lane == 0)
                for (int k = 0; k < rep; ++k) t->lens[i + k] = (uint8_t)val;
            i += rep;
            prev = val;
        }
    }
    if (ctx.lane == 0) {
        int st = t->lens[256] == 0 ? GV_PNG_BAD_CODES : GV_PNG_OK;       // no end-of-block code
        if (st == GV_PNG_OK) st = gv_png_build(lit, t->lens, hlit, 1, t->offs);
        if (st == GV_PNG_OK) st = gv_png_build(dst, t->lens + hlit, hdist, 2, t->offs);
        t->status = st;
    }
    ctx.sync();
    return (int)ctx.uni((uint32_t)t->status);
}

// Adler-32 of out[0, n): the lanes take 256-byte pieces in turn; a piece at offset o with sums (a, b) adds a to the low
// half and b + (n - o - len) * a to the high half.
template <class Ctx>
GV_PNG_HD uint32_t gv_png_adler32(const uint8_t* out, uint32_t n, GvPngTables* t, const Ctx& ctx) {
    uint32_t sa = 0, sb = 0;
    for (uint32_t o = (uint32_t)ctx.lane * 256u; o < n; o += (uint32_t)ctx.nlanes * 256u) {
        const uint32_t len = n - o < 256u ? n - o : 256u;
        uint32_t a = 0, bb = 0;
        for (uint32_t k = 0; k < len; ++k) {
            a += out[o + k];
            bb += a;
        }
        sa = (sa + a) % 65521u;
        sb = (sb + bb % 65521u + ((n - o - len) % 65521u) * a % 65521u) % 65521u;
    }
    ctx.sync();
    t->red[2 * ctx.lane] = sa;
    t->red[2 * ctx.lane + 1] = sb;
    ctx.sync();
    uint32_t a = 1, b = n % 65521u;                              // the leading 1 of the low half is added n times
    for (int l = 0; l < ctx.nlanes; ++l) {
        a = (a + ctx.uni(t->red[2 * l])) % 65521u;
        b = (b + ctx.uni(t->red[2 * l + 1])) % 65521u;
    }
    return b << 16 | a;
}

// zlib stream in[0, in_len) -> out[0, out_size) exactly.  GV_PNG_OK or the first error met.
template <class Ctx>
GV_PNG_HD int gv_png_inflate(const uint8_t* in, uint32_t in_len, uint8_t* out, uint32_t out_size, GvPngTables* t,
                             const Ctx& ctx) {
    if (in_len < 2) return GV_PNG_TRUNCATED;
    const int cmf = (int)ctx.uni(in[0]), flg = (int)ctx.uni(in[1]);
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) return GV_PNG_BAD_HEADER;
    GvPngBits b = {in, in_len, 2u, 0ull, 0, 0u};
    gv_png_seek(b, 2u, ctx);
    const GvPngHuff lit = {t->lfast, t->lsym, t->lcount, GV_PNG_LFAST};
    const GvPngHuff dst = {t->dfast, t->dsym, t->dcount, GV_PNG_DFAST};
    uint32_t op = 0;
    for (;;) {
        const int fin = gv_png_bits(b, 1, ctx), type = gv_png_bits(b, 2, ctx);
        if (fin < 0 || type < 0) return GV_PNG_TRUNCATED;
        if (type == 3) return GV_PNG_BAD_BLOCK;
        if (type == 0) {
            b.buf >>= b.cnt & 7;                                 // to the byte boundary
            b.cnt -= b.cnt & 7;
            const int len = gv_png_bits(b, 16, ctx), nlen = gv_png_bits(b, 16, ctx);
            if (len < 0 || nlen < 0) return GV_PNG_TRUNCATED;
            if ((len ^ 0xffff) != nlen) return GV_PNG_BAD_BLOCK;
            gv_png_seek(b, b.pos - (uint32_t)(b.cnt >> 3), ctx);         // hand the whole bytes read ahead back
            if ((uint32_t)len > b.len - b.pos) return GV_PNG_TRUNCATED;
            if ((uint32_t)len > out_size - op) return GV_PNG_TOO_LONG;
            for (uint32_t left = (uint32_t)len; left;) {
                const uint32_t run = left < ctx.max_run() ? left : ctx.max_run();
                for (uint32_t k = (uint32_t)ctx.lane; k < run; k += (uint32_t)ctx.nlanes) ctx.put(out, op + k, in[b.pos + k]);
                gv_png_seek(b, b.pos + run, ctx);
                op += run;
                left -= run;
                ctx.wrote(out, op - run, op);
            }
        } else {
            const int st = gv_png_block_tables(b, type, t, ctx);
            if (st != GV_PNG_OK) return st;
            for (;;) {
                int s = gv_png_symbol(b, lit, ctx);
                if (s < 0) return -s;
                if (s < 256) {
                    if (op >= out_size) return GV_PNG_TOO_LONG;
                    if (ctx.lane == 0) ctx.put(out, op, (uint8_t)s);
                    ++op;
                    ctx.wrote(out, op - 1, op);
                    continue;
                }
                if (s == 256) break;
                if (s > 285) return GV_PNG_BAD_CODES;
                int len, eb;
                if (s < 265) { len = s - 254; eb = 0; }
                else if (s == 285) { len = 258; eb = 0; }
                else { eb = (s - 261) >> 2; len = 3 + ((4 + ((s - 261) & 3)) << eb); }
                if (eb) {
                    const int x = gv_png_bits(b, eb, ctx);
                    if (x < 0) return GV_PNG_TRUNCATED;
                    len += x;
                }
                s = gv_png_symbol(b, dst, ctx);
                if (s < 0) return -s;
                if (s > 29) return GV_PNG_BAD_CODES;
                int dist = s + 1;
                if (s >= 4) {
                    eb = (s >> 1) - 1;
                    const int x = gv_png_bits(b, eb, ctx);
                    if (x < 0) return GV_PNG_TRUNCATED;
                    dist = 1 + ((2 + (s & 1)) << eb) + x;
                }
                if ((uint32_t)dist > op) return GV_PNG_BAD_DISTANCE;
                if ((uint32_t)len > out_size - op) return GV_PNG_TOO_LONG;
                // The window is the output already written.  Byte k of the match is byte k % dist of the dist bytes in
                // front of it (an overlapping match, dist < len, repeats them): every source byte was written BEFORE this
                // match, so the lanes can copy in any order once those writes are visible to the group.
                ctx.sync();
                const uint32_t src = op - (uint32_t)dist;
                if (dist >= len) {
                    for (int k = ctx.lane; k < len; k += ctx.nlanes) ctx.put(out, op + (uint32_t)k, ctx.get(out, src + (uint32_t)k));
                } else {
                    for (int k = ctx.lane; k < len; k += ctx.nlanes)
                        ctx.put(out, op + (uint32_t)k, ctx.get(out, src + (uint32_t)(k % dist)));
                }
                op += (uint32_t)len;
                ctx.wrote(out, op - (uint32_t)len, op);
            }
        }
        if (fin) break;
    }
    if (op != out_size) return GV_PNG_TOO_SHORT;
    ctx.finish(out, op);
    b.pos -= (uint32_t)(b.cnt >> 3);                              // the trailer starts on the next byte boundary
    if (b.len - b.pos < 4) return GV_PNG_TRUNCATED;
    const uint8_t* tr = in + b.pos;
    const uint32_t want = ctx.uni((uint32_t)tr[0] << 24 | (uint32_t)tr[1] << 16 | (uint32_t)tr[2] << 8 | tr[3]);
    ctx.sync();
    return gv_png_adler32(out, out_size, t, ctx) == want ? GV_PNG_OK : GV_PNG_BAD_CHECKSUM;
}

GV_PNG_HD int gv_png_paeth(int a, int b, int c) {
    const int pa = b > c ? b - c : c - b, pb = a > c ? a - c : c - a;
    int pc = a + b - 2 * c;
    pc = pc < 0 ? -pc : pc;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// The serial un-filter + expand of the host twin: raw = h rows of (filter byte + w * ch bytes), un-filtered IN PLACE,
// then written as [h, w, 3] with tf.image.decode_png(channels=3) semantics (gray replicated, alpha dropped, PLTE
// lookup; pal: plen RGB triples).
inline int gv_png_unfilter_expand_serial(uint8_t* raw, int h, int w, int ctype, const uint8_t* pal, int plen,
                                         uint8_t* out) {
    const int bpp = gv_png_channels(ctype), rb = w * bpp;
    for (int y = 0; y < h; ++y) {
        uint8_t* cur = raw + (size_t)y * (rb + 1) + 1;
        const uint8_t* prev = y ? cur - (rb + 1) : nullptr;
        const int ft = cur[-1];
        if (ft > 4) return GV_PNG_BAD_FILTER;
        for (int x = 0; x < rb && ft; ++x) {
            const int a = x >= bpp ? cur[x - bpp] : 0, bb = prev ? prev[x] : 0, c = (prev && x >= bpp) ? prev[x - bpp] : 0;
            const int p = ft == 1 ? a : ft == 2 ? bb : ft == 3 ? (a + bb) >> 1 : gv_png_paeth(a, bb, c);
            cur[x] = (uint8_t)(cur[x] + p);
        }
        uint8_t* o = out + (size_t)y * w * 3;
        for (int x = 0; x < w; ++x) {
            const uint8_t* p = cur + x * bpp;
            if (ctype == 3) {
                if (p[0] >= plen) return GV_PNG_BAD_PALETTE_INDEX;
                p = pal + 3 * p[0];
            }
            const int rgb = ctype == 2 || ctype == 6 || ctype == 3;
            o[3 * x] = p[0];
            o[3 * x + 1] = rgb ? p[1] : p[0];
            o[3 * x + 2] = rgb ? p[2] : p[0];
        }
    }
    return GV_PNG_OK;
}
