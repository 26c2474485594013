// Stand-alone host program over the boundary tracer's shared per-edge rule (csrc/contour_dev.h: the source the kernels of contour.hip
// compile).  tests/test_contours_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it over a corpus
// it wrote; it is never loaded into python.  It walks a map the way the kernels' lanes do - one Quad per corner for the leaving edges
// and vertex flags, one Quad at the head corner and a bisection of the keys per edge for its successor, then the doubling rounds, the
// leaders, the ranks and the three prefix sums in the kernels' own arithmetic - so UBSan sees every product and sum the device forms,
// and ASan every index into the map (allocated to its last row's last byte, no slack) and the per-edge arrays.
//   usage: contour_san CORPUS RESULTS
//   CORPUS : u32 cases, then per case i32 W, H, ox, oy, sx, sy, bounds_w, bounds_h (0: no clamp), shift (bytes before the map's first
//            byte), pitch; 256 bytes traced table; H x W map bytes
//   RESULTS: per case u32 n_edges, n_loops, n_vertices; n_vertices x 2 i32; n_loops x 8 i32 records; n_loops x i64 area2
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../wsi_segmentation_pipeline_amd/csrc/contour_dev.h"

using namespace wsi_contour;

static bool read_n(FILE* f, void* v, size_t bytes) { return bytes == 0 || fread(v, bytes, 1, f) == 1; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CORPUS RESULTS\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    unsigned cases = 0;
    if (!read_n(in, &cases, 4)) return 2;
    for (unsigned c = 0; c < cases; ++c) {
        int head[10];
        unsigned char table[256];
        if (!read_n(in, head, sizeof head) || !read_n(in, table, 256)) return 2;
        const int W = head[0], H = head[1], ox = head[2], oy = head[3], sx = head[4], sy = head[5], bw = head[6], bh = head[7], shift = head[8];
        const long long pitch = head[9];
        if (W < 1 || H < 1 || (long long)W * H > MAX_PIXELS || pitch < W || shift < 0 || sx < 1 || sy < 1) return 2;
        const size_t bytes = (size_t)shift + (size_t)(H - 1) * pitch + W;
        unsigned char* buf = (unsigned char*)malloc(bytes);
        memset(buf, 0xA5, bytes);
        const unsigned char* map = buf + shift;
        for (int y = 0; y < H; ++y) if (!read_n(in, buf + shift + y * pitch, W)) return 2;
        Traced tr{};
        for (int l = 0; l < 256; ++l) if (table[l]) tr.bits[l >> 5] |= 1u << (l & 31);

        // count + build: keys in key order, vertex flags
        std::vector<uint32_t> key;
        std::vector<unsigned char> flag;
        for (long long ty = 0; ty <= H; ++ty)
            for (long long tx = 0; tx <= W; ++tx) {
                const Quad q = quad_at(map, pitch, W, H, tx, ty);
                const unsigned m = leaving_mask(q, tr);
                for (int d = 0; d < 4; ++d)
                    if ((m >> d) & 1u) {
                        key.push_back((uint32_t)((ty * ((long long)W + 1) + tx) * 4 + d));
                        flag.push_back(tail_is_vertex(q, d));
                    }
            }
        const uint32_t n = (uint32_t)key.size();
        std::vector<uint32_t> succ(n), jump[2] = {std::vector<uint32_t>(n), std::vector<uint32_t>(n)};
        std::vector<uint64_t> word[2] = {std::vector<uint64_t>(n), std::vector<uint64_t>(n)};
        for (uint32_t e = 0; e < n; ++e) {
            const int d = (int)(key[e] & 3u);
            const long long hc = head_corner((long long)(key[e] >> 2), d, W);
            const Quad q = quad_at(map, pitch, W, H, hc % ((long long)W + 1), hc / ((long long)W + 1));
            const uint32_t want = (uint32_t)(hc * 4 + next_heading(q, d));
            uint32_t lo = 0, hi = n;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (key[mid] < want) lo = mid + 1; else hi = mid;
            }
            if (lo >= n || key[lo] != want) { fprintf(stderr, "case %u: edge %u has no successor\n", c, e); return 3; }
            succ[e] = jump[0][e] = lo;
            word[0][e] = (uint64_t)e << 32;
        }
        int rounds = 0;
        while ((1LL << rounds) < (long long)n) ++rounds;
        for (int k = 0; k < rounds; ++k)
            for (uint32_t e = 0; e < n; ++e) {
                const uint32_t j = jump[k & 1][e];
                const uint64_t own = word[k & 1][e], far = word[k & 1][j] + (1u << k);
                word[(k + 1) & 1][e] = own < far ? own : far;
                jump[(k + 1) & 1][e] = jump[k & 1][j];
            }
        const std::vector<uint64_t>& wd = word[rounds & 1];
        // leaders, loop index and first slot (one u64 prefix sum), then every edge to its slot
        std::vector<uint64_t> X(n), S(n + 1), cross(n), CS(n + 1);
        std::vector<uint32_t> okey(n), oflag(n), VS(n + 1);
        for (uint32_t e = 0; e < n; ++e) X[e] = (uint32_t)wd[e] == 0u ? (1ull << 32) | (uint64_t)((uint32_t)wd[succ[e]] + 1u) : 0ull;
        S[0] = 0;
        for (uint32_t e = 0; e < n; ++e) S[e + 1] = S[e] + X[e];
        for (uint32_t e = 0; e < n; ++e) {
            const uint32_t leader = (uint32_t)(wd[e] >> 32), dist = (uint32_t)wd[e], len = (uint32_t)X[leader];
            if (len == 0) { fprintf(stderr, "case %u: edge %u has no leader\n", c, e); return 3; }
            const uint64_t pos = (uint64_t)(uint32_t)S[leader] + (len - dist % len) % len;
            const long long corner = (long long)(key[e] >> 2);
            okey.at(pos) = key[e];
            oflag.at(pos) = flag[e];
            cross.at(pos) = (uint64_t)cross_term(corner % ((long long)W + 1), corner / ((long long)W + 1), (int)(key[e] & 3u));
        }
        VS[0] = 0;
        CS[0] = 0;
        for (uint32_t p = 0; p < n; ++p) { VS[p + 1] = VS[p] + oflag[p]; CS[p + 1] = CS[p] + cross[p]; }
        const uint32_t n_loops = (uint32_t)(S[n] >> 32), n_vertices = VS[n];
        std::vector<int> vertices(2 * (size_t)n_vertices), recs(8 * (size_t)n_loops, 0);
        std::vector<long long> area2(n_loops);
        for (uint32_t p = 0; p < n; ++p)
            if (oflag[p]) {
                const long long corner = (long long)(okey[p] >> 2);
                vertices.at(2 * (size_t)VS[p]) = level0(corner % ((long long)W + 1), ox, sx, bw);
                vertices.at(2 * (size_t)VS[p] + 1) = level0(corner / ((long long)W + 1), oy, sy, bh);
            }
        for (uint32_t e = 0; e < n; ++e)
            if (X[e]) {
                const uint32_t len = (uint32_t)X[e], loop = (uint32_t)(S[e] >> 32), first = (uint32_t)S[e];
                const long long corner = (long long)(key[e] >> 2);
                const Quad q = quad_at(map, pitch, W, H, corner % ((long long)W + 1), corner / ((long long)W + 1));
                int* r = &recs.at(8 * (size_t)loop);
                r[0] = (int)VS.at(first);
                r[1] = (int)(VS.at(first + len) - VS[first]);
                r[2] = (int)len;
                r[3] = edge_label(q, (int)(key[e] & 3u));
                area2.at(loop) = (long long)(CS.at(first + len) - CS[first]);
            }
        const unsigned counts[3] = {n, n_loops, n_vertices};
        fwrite(counts, 4, 3, out);
        if (n_vertices) fwrite(vertices.data(), 4, vertices.size(), out);
        if (n_loops) { fwrite(recs.data(), 4, recs.size(), out); fwrite(area2.data(), 8, area2.size(), out); }
        free(buf);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
