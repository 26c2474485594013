// Stand-alone host program over the annotation rasteriser's shared coverage test (csrc/poly_dev.h: the source the kernel of poly.hip
// compiles).  tests/test_annotations_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it over a
// corpus it wrote; it is never loaded into python.  It walks a map the way the kernel's lanes do - rows cut into aligned 16-byte
// pieces at a given address offset, one edge_run per edge and piece, paint16 per polygon - so UBSan's signed-overflow check sees
// every product and sum the device forms, and ASan every index into the map, the edges and the records.
//   usage: poly_san CORPUS RESULTS
//   CORPUS : u32 cases, then per case i32 W, H, ox, oy, sx, sy, shift (address of the map's first byte mod 16), pitch, fill (the
//            byte the map holds before), n_polys, n_edges; n_polys x 8 i32 records; n_edges x 4 i32 edges
//   RESULTS: per case i32 status (0; 1: a record leaves the edge array), then H x W bytes
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../wsi_segmentation_pipeline_amd/csrc/poly_dev.h"

using namespace wsi_poly;

static bool read_n(FILE* f, void* v, size_t bytes) { return bytes == 0 || fread(v, bytes, 1, f) == 1; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CORPUS RESULTS\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    unsigned cases = 0;
    if (!read_n(in, &cases, 4)) return 2;
    for (unsigned c = 0; c < cases; ++c) {
        int head[11];
        if (!read_n(in, head, sizeof head)) return 2;
        const int W = head[0], H = head[1], ox = head[2], oy = head[3], sx = head[4], sy = head[5], shift0 = head[6], pitch = head[7], fill = head[8];
        const int n_polys = head[9], n_edges = head[10];
        if (W <= 0 || H <= 0 || n_polys < 0 || n_edges < 0 || pitch < W) return 2;
        PolyRec* polys = (PolyRec*)malloc(n_polys ? sizeof(PolyRec) * n_polys : 1);
        int* edges = (int*)malloc(n_edges ? sizeof(int) * 4 * n_edges : 1);
        unsigned char* map = (unsigned char*)malloc((size_t)W * H);
        if (!read_n(in, polys, sizeof(PolyRec) * n_polys) || !read_n(in, edges, sizeof(int) * 4 * n_edges)) return 2;
        memset(map, fill, (size_t)W * H);
        int status = 0;
        for (int y = 0; y < H; ++y) {
            const int shift = (int)((shift0 + (long long)y * pitch) & 15);
            const long long runs = ((long long)W + shift + RUN - 1) / RUN;
            const int py = (int)(oy + (long long)y * sy);
            for (long long r = 0; r < runs; ++r) {
                int kbeg, kend;
                const long long x0 = lane_run(r, shift, W, &kbeg, &kend);
                if (kend <= kbeg) continue;
                const int px_first = (int)(ox + (x0 + kbeg) * sx);
                uint32_t word[4] = {0u, 0u, 0u, 0u};
                for (int k = kbeg; k < kend; ++k) word[k >> 2] |= (uint32_t)map[(size_t)y * W + x0 + k] << (8 * (k & 3));
                for (int p = 0; p < n_polys; ++p) {
                    const PolyRec& rec = polys[p];
                    if (rec.first < 0 || rec.count <= 0 || (long long)rec.first + rec.count > n_edges) { status = 1; continue; }
                    unsigned odd = 0, on = 0;
                    for (int i = 0; i < rec.count; ++i) {
                        const int* v = edges + 4 * ((size_t)rec.first + i);
                        const Edge e = edge_sorted(v[0], v[1], v[2], v[3]);
                        if (kend - kbeg == RUN) edge_run<true>(e, px_first, sx, py, 0, RUN, &odd, &on);
                        else edge_run<false>(e, px_first, sx, py, kbeg, kend, &odd, &on);
                    }
                    paint16(word, odd | on, (unsigned)rec.label & 255u);
                }
                for (int k = kbeg; k < kend; ++k) map[(size_t)y * W + x0 + k] = (unsigned char)(word[k >> 2] >> (8 * (k & 3)));
            }
        }
        fwrite(&status, 4, 1, out);
        fwrite(map, 1, (size_t)W * H, out);
        free(map);
        free(edges);
        free(polys);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
