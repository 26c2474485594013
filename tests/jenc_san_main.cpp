// Stand-alone host program over the JPEG encoder's shared per-tile entropy loop (csrc/jpeg_enc_dev.h: the source the size and write
// kernels compile).  tests/test_jpeg_enc_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it over
// a corpus it wrote; it is never loaded into python.
//   usage: jenc_san CORPUS RESULTS
//   CORPUS : u32 cases, then per case i32 width, height, ncomp, hs, vs, restart, u32 n, n int16 coefficients (MCU order, zigzag)
//   RESULTS: per case i32 status (0; 1: the geometry is refused or n is not its coefficient count; 2: the passes disagree), u32 size,
//            the scan bytes
// The coefficients and the scan live in heap blocks of exactly their size - the scan's is the size pass's answer - so a read or
// write one byte outside either is reported.
#include <stdio.h>
#include <stdlib.h>
#include "../wsi_segmentation_pipeline_amd/csrc/jpeg_enc_dev.h"

static bool read_n(FILE* f, void* v, size_t bytes) { return bytes == 0 || fread(v, bytes, 1, f) == 1; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CORPUS RESULTS\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    static const wsi_jenc::EncTables tables = wsi_jenc::make_enc_tables();
    unsigned cases = 0;
    if (!read_n(in, &cases, 4)) return 2;
    for (unsigned c = 0; c < cases; ++c) {
        int head[6];
        unsigned n = 0;
        if (!read_n(in, head, sizeof head) || !read_n(in, &n, 4)) return 2;
        short* coef = (short*)malloc(n ? (size_t)n * 2 : 1);
        if (!read_n(in, coef, (size_t)n * 2)) return 2;
        wsi_jenc::Geometry g;
        int status = 0;
        unsigned size = 0;
        unsigned char* scan = nullptr;
        if (!wsi_jenc::geometry_make(head[0], head[1], head[2], head[3], head[4], &g) || (long long)n != g.coefs) {
            status = 1;
        } else {
            size = (unsigned)wsi_jenc::encode_tile(coef, g, head[5], tables.code, wsi_jenc::CountSink());
            scan = (unsigned char*)malloc(size ? size : 1);
            wsi_jenc::StoreSink sink;
            sink.p = scan;
            sink.cap = size;
            if (wsi_jenc::encode_tile(coef, g, head[5], tables.code, sink) != size) status = 2;
        }
        fwrite(&status, 4, 1, out);
        fwrite(&size, 4, 1, out);
        if (size) fwrite(scan, 1, size, out);
        free(scan);
        free(coef);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
