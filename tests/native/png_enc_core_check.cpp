// Stand-alone host check of csrc/png_enc_core.h for a sanitizer build (no GPU, no Python at run time):
//     python tests/png_enc_cases.py DIR/enc.bin
//     g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Igvcnn-tf_amd/csrc
//         tests/native/png_enc_core_check.cpp -o png_enc_core_check && ./png_enc_core_check DIR/enc.bin
// Every record (tests/png_enc_cases.py: dump) is encoded from and into buffers of EXACTLY the sizes the ABI asks for (the
// pixels; gv_png_enc_bound bytes of output), so a read or write one byte out of bounds is a sanitizer report.  The
// stream is then inflated by the host decoder of csrc/png_core.h into a buffer of exactly the raw size and compared
// with the record's expected raw stream (filter bytes and filtered rows) and colour type.  Exit code 0: all records ran
// and every expectation held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "png_enc_core.h"

int main(int argc, char** argv) {
    long total = 0, wrong = 0, in_bytes = 0, out_bytes = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        int32_t head[6];
        while (fread(head, sizeof(head), 1, f) == 1) {
            const int w = head[0], h = head[1], filter = head[2], color = head[3], want_type = head[4], rawlen = head[5];
            if (w <= 0 || h <= 0 || rawlen <= 0 || gv_png_enc_raw_bytes(h, w, 3) > 0x7fffffff) {
                fprintf(stderr, "%s: bad record header\n", argv[a]);
                return 2;
            }
            const size_t npix = (size_t)h * w * 3;
            uint8_t* pix = (uint8_t*)malloc(npix);
            uint8_t* want = (uint8_t*)malloc((size_t)rawlen);
            if (fread(pix, 1, npix, f) != npix || fread(want, 1, (size_t)rawlen, f) != (size_t)rawlen) {
                fprintf(stderr, "%s: short record\n", argv[a]);
                return 2;
            }
            const int64_t cap = gv_png_enc_bound(h, w);
            uint8_t* out = (uint8_t*)malloc((size_t)cap);
            uint32_t* rows = (uint32_t*)malloc(((size_t)gv_png_enc_raw_bytes(h, w, 3) + 3) / 4 * 4);
            uint32_t* slot = (uint32_t*)malloc(GV_PNG_ENC_SEGOUT);
            GvPngEncSeg* seg = (GvPngEncSeg*)malloc(sizeof(GvPngEncSeg));
            memset(seg, 0xA5, sizeof(*seg));                     // stale state of "the previous segment"
            int32_t length = -1, ctype = -1;
            int st = gv_png_enc_image_serial(pix, h, w, filter, color, (uint8_t*)rows, (uint8_t*)slot, seg, out, cap, &length, &ctype);
            const char* why = nullptr;
            if (st != GV_PNG_OK) why = "encoder status";
            else if (ctype != want_type) why = "colour type";
            else if (length < 6 || length > cap) why = "length";
            else if (gv_png_enc_raw_bytes(h, w, ctype == 0 ? 1 : 3) != rawlen) why = "raw size";
            if (!why) {
                uint8_t* raw = (uint8_t*)malloc((size_t)rawlen);
                uint8_t* exact = (uint8_t*)malloc((size_t)length);       // (the decoder may not read past `length` either)
                memcpy(exact, out, (size_t)length);
                GvPngTables* t = (GvPngTables*)malloc(sizeof(GvPngTables));
                memset(t, 0xA5, sizeof(*t));
                st = gv_png_inflate(exact, (uint32_t)length, raw, (uint32_t)rawlen, t, GvPngHostCtx());
                if (st != GV_PNG_OK) why = "the stream does not inflate (GV_PNG_* below)";
                else if (memcmp(raw, want, (size_t)rawlen)) why = "raw stream differs";
                free(raw);
                free(exact);
                free(t);
                out_bytes += length;
                in_bytes += rawlen;
            }
            if (why) {
                fprintf(stderr, "%s record %ld (%dx%d filter %d colour %d): %s, status %d\n", argv[a], total, w, h, filter, color, why, st);
                ++wrong;
            }
            ++total;
            free(pix);
            free(want);
            free(out);
            free(rows);
            free(slot);
            free(seg);
        }
        fclose(f);
    }
    printf("%ld records, %ld wrong; %ld raw bytes -> %ld stream bytes\n", total, wrong, in_bytes, out_bytes);
    return wrong || !total ? 1 : 0;
}
