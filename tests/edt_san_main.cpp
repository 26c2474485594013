// Stand-alone host program over the distance transform's shared per-column step and per-pixel scan (csrc/edt_dev.h: the source the
// kernels of edt.hip compile).  tests/test_edt_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it
// over a corpus it wrote; it is never loaded into python.  It walks a map the way the kernels' lanes do - per column the bands'
// first and last feature rows, the walk over the bands down and up, then every band alone from its two carries; per row scan_pixel
// over a copy of the row that is exactly W values long - so UBSan sees every product and sum the device forms, and ASan every index
// into the map (allocated to its last row's last byte, no slack), the band tables and the row.
//   usage: edt_san CORPUS RESULTS
//   CORPUS : u32 cases, then per case i32 kind, W, H, invert, shift (bytes before the map's first byte), pitch; then
//            kind 0: H x W map bytes; kind 1 (H = 1): W u16, a hand-made row of the g plane
//   RESULTS: per case of kind 0 H x W u16 (g), then H x W i32 (out); per case of kind 1 W i32
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../wsi_segmentation_pipeline_amd/csrc/edt_dev.h"

using namespace wsi_edt;

static bool read_n(FILE* f, void* v, size_t bytes) { return bytes == 0 || fread(v, bytes, 1, f) == 1; }

static void rows_of(const std::vector<uint16_t>& plane, int W, int H, std::vector<int32_t>& out) {
    out.assign((size_t)W * H, 0);
    for (int y = 0; y < H; ++y) {
        const std::vector<uint16_t> row(plane.begin() + (size_t)y * W, plane.begin() + (size_t)(y + 1) * W);
        bool finite = false;
        for (int x = 0; x < W; ++x) finite = finite || row[x] != G_NONE;
        for (int x = 0; x < W; ++x) out[(size_t)y * W + x] = finite ? scan_pixel(row.data(), W, x) : EDT_NONE;
    }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CORPUS RESULTS\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    unsigned cases = 0;
    if (!read_n(in, &cases, 4)) return 2;
    for (unsigned c = 0; c < cases; ++c) {
        int head[6];
        if (!read_n(in, head, sizeof head)) return 2;
        const int kind = head[0], W = head[1], H = head[2], invert = head[3], shift = head[4];
        const long long pitch = head[5];
        if (W < 1 || H < 1 || W > LIMIT || H > LIMIT || shift < 0 || kind < 0 || kind > 1) return 2;
        std::vector<int32_t> d2;
        if (kind == 1) {
            if (H != 1) return 2;
            std::vector<uint16_t> plane((size_t)W);
            if (!read_n(in, plane.data(), (size_t)W * 2)) return 2;
            rows_of(plane, W, 1, d2);
            fwrite(d2.data(), 4, d2.size(), out);
            continue;
        }
        if (pitch < W) return 2;
        const size_t bytes = (size_t)shift + (size_t)(H - 1) * pitch + W;
        unsigned char* buf = (unsigned char*)malloc(bytes);
        memset(buf, 0xA5, bytes);
        const unsigned char* map = buf + shift;
        for (int y = 0; y < H; ++y) if (!read_n(in, buf + shift + y * pitch, W)) return 2;

        const int nb = bands(H);
        if (workspace_bytes(W, H) != plane_bytes(W, H) + 2 * summary_bytes(W, H) || summary_bytes(W, H) < (size_t)nb * W * 4) return 3;
        std::vector<int> first_tab((size_t)nb * W), last_tab((size_t)nb * W);
        for (int b = 0; b < nb; ++b)                            // the band summaries
            for (int x = 0; x < W; ++x) {
                int first = -1, last = -1;
                for (int y = b * BAND; y < H && y < (b + 1) * BAND; ++y) band_rows(is_feature(map[y * pitch + x], invert), y, &first, &last);
                first_tab.at((size_t)b * W + x) = first;
                last_tab.at((size_t)b * W + x) = last;
            }
        for (int x = 0; x < W; ++x) {                           // the carries
            int carry = -1;
            for (int b = 0; b < nb; ++b) carry_down(&last_tab.at((size_t)b * W + x), &carry);
            carry = -1;
            for (int b = nb - 1; b >= 0; --b) carry_up(&first_tab.at((size_t)b * W + x), &carry);
        }
        std::vector<uint16_t> plane((size_t)W * H);
        for (int b = 0; b < nb; ++b) {                          // every band alone
            const int y0 = b * BAND, rows = H - y0 < BAND ? H - y0 : BAND;
            std::vector<uint16_t> down((size_t)rows);
            for (int x = 0; x < W; ++x) {
                uint16_t d = carry_distance(last_tab.at((size_t)b * W + x), y0 - 1);
                for (int j = 0; j < rows; ++j) {
                    d = column_step(d, is_feature(map[(long long)(y0 + j) * pitch + x], invert));
                    down.at(j) = d;
                }
                d = carry_distance(first_tab.at((size_t)b * W + x), y0 + rows);
                for (int j = rows - 1; j >= 0; --j) {
                    const uint16_t dn = down.at(j);
                    d = column_step(d, dn == 0);
                    plane.at((size_t)(y0 + j) * W + x) = dn < d ? dn : d;
                }
            }
        }
        rows_of(plane, W, H, d2);
        fwrite(plane.data(), 2, plane.size(), out);
        fwrite(d2.data(), 4, d2.size(), out);
        free(buf);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
