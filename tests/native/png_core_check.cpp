// Stand-alone host check of csrc/png_core.h for a sanitizer build (no GPU, no Python):
//     python tests/png_cases.py DIR
//     g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Igvcnn-tf_amd/csrc
//         tests/native/png_core_check.cpp -o png_core_check && ./png_core_check DIR/good.bin DIR/malformed.bin DIR/flips.bin
// Every record (tests/png_cases.py: dump) is decoded from buffers of EXACTLY its size, so a read or write one byte out
// of bounds is a sanitizer report; a record with an expected status must return it.  Exit code 0: all records ran and
// every expectation held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "png_core.h"

int main(int argc, char** argv) {
    long total = 0, wrong = 0, by_status[16] = {};
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        int32_t head[6];
        while (fread(head, sizeof(head), 1, f) == 1) {
            const int w = head[0], h = head[1], ctype = head[2], plen = head[3], expect = head[4], slen = head[5];
            const int ch = gv_png_channels(ctype);
            if (w <= 0 || h <= 0 || !ch || plen < 0 || plen > 256 || slen < 0) {
                fprintf(stderr, "%s: bad record header\n", argv[a]);
                return 2;
            }
            uint8_t* pal = (uint8_t*)malloc(plen ? plen * 3 : 1);
            uint8_t* in = (uint8_t*)malloc(slen ? slen : 1);
            if ((plen && fread(pal, 3, plen, f) != (size_t)plen) || (slen && fread(in, 1, slen, f) != (size_t)slen)) {
                fprintf(stderr, "%s: short record\n", argv[a]);
                return 2;
            }
            const size_t raw_size = (size_t)h * (1 + (size_t)w * ch);
            uint8_t* raw = (uint8_t*)malloc(raw_size);
            uint8_t* out = (uint8_t*)malloc((size_t)h * w * 3);
            GvPngTables* t = (GvPngTables*)malloc(sizeof(GvPngTables));
            memset(t, 0xA5, sizeof(*t));                          // stale tables of "the previous image"
            int st = gv_png_inflate(in, (uint32_t)slen, raw, (uint32_t)raw_size, t, GvPngHostCtx());
            if (st == GV_PNG_OK) st = gv_png_unfilter_expand_serial(raw, h, w, ctype, pal, plen, out);
            if (st < 0 || st > GV_PNG_BAD_PALETTE_INDEX) {
                fprintf(stderr, "%s record %ld: status %d is not a GV_PNG_* value\n", argv[a], total, st);
                return 1;
            }
            by_status[st]++;
            if (expect >= 0 && st != expect) {
                fprintf(stderr, "%s record %ld: status %d, expected %d\n", argv[a], total, st, expect);
                ++wrong;
            }
            ++total;
            free(pal);
            free(in);
            free(raw);
            free(out);
            free(t);
        }
        fclose(f);
    }
    printf("%ld records, %ld wrong; by status:", total, wrong);
    for (int s = 0; s <= GV_PNG_BAD_PALETTE_INDEX; ++s) printf(" %d:%ld", s, by_status[s]);
    printf("\n");
    return wrong ? 1 : 0;
}
