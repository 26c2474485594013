// Stand-alone host program over the JPEG path's host side and its shared per-tile decode loop (csrc/jpeg_walk.h, csrc/jpeg_dev.h: the
// source the entropy kernel compiles).  tests/test_jpeg_cpu.py builds it with the host compiler under -fsanitize=address,undefined
// and runs it over a corpus it wrote; it is never loaded into python.
//   usage: jpeg_san CORPUS RESULTS
//   CORPUS : u32 cases, then per case u32 tables_len, tables, u32 stream_len, stream
//   RESULTS: per case i32 status (the walk's, else the decode's), i32 n (int16 coefficients that follow; 0 unless status 0), the coefficients
// Every stream and every coefficient area lives in a heap block of exactly its size, so a read or write one byte outside it is reported.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../wsi_segmentation_pipeline_amd/csrc/jpeg_walk.h"

static bool read_u32(FILE* f, unsigned* v) { return fread(v, 4, 1, f) == 1; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CORPUS RESULTS\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    unsigned cases = 0;
    if (!read_u32(in, &cases)) return 2;
    std::vector<wsi_jpeg_tables> sets(4);
    for (unsigned c = 0; c < cases; ++c) {
        unsigned tlen = 0, slen = 0;
        if (!read_u32(in, &tlen)) return 2;
        unsigned char* tables = (unsigned char*)malloc(tlen ? tlen : 1);
        if (tlen && fread(tables, 1, tlen, in) != tlen) return 2;
        if (!read_u32(in, &slen)) return 2;
        unsigned char* stream = (unsigned char*)malloc(slen ? slen : 1);
        if (slen && fread(stream, 1, slen, in) != slen) return 2;

        wsi_jpeg_tables base;
        int status = 0;
        if (tlen) status = wsi_jpeg::parse_tables(tables, tlen, &base);
        wsi_jpeg_tile rec;
        int n_sets = 0;
        short* coef = nullptr;
        int ncoef = 0;
        if (status == 0) {
            const unsigned long long off = 0;
            if (wsi_jpeg::walk(stream, slen, &off, &slen, 1, tlen ? &base : nullptr, sets.data(), (int)sets.size(), &n_sets, &rec) != 0) return 3;
            status = rec.status;
        }
        if (status == 0) {
            wsi_jpeg::Geometry g;
            if (!wsi_jpeg::geometry_make(rec.width, rec.height, rec.ncomp, rec.h[0], rec.v[0], &g) || !wsi_jpeg::tile_matches(rec, g)) {
                status = WSI_JPEG_GEOMETRY;
            } else {
                coef = (short*)calloc((size_t)g.coefs, sizeof(short));
                ncoef = (int)g.coefs;
                status = wsi_jpeg::decode_tile(stream, rec, &sets[rec.table_set], g, coef);
            }
        }
        const int n_out = status == 0 ? ncoef : 0;
        fwrite(&status, 4, 1, out);
        fwrite(&n_out, 4, 1, out);
        if (n_out) fwrite(coef, sizeof(short), (size_t)n_out, out);
        free(coef);
        free(stream);
        free(tables);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
