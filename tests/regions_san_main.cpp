// Stand-alone host program over the region tables' shared per-run arithmetic (csrc/regions_dev.h: the source the kernels of regions.hip
// compile).  tests/test_regions_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs it over a corpus it
// wrote; it is never loaded into python.  It walks a map the way the kernels' lanes do - starts and ends per chunk of CHUNK pixels of a
// row with the neighbour bytes of the adjoining chunks, the scan of the chunk sums, a start and the end pixel of a run writing the same
// record, one step per run bisecting the row above and uniting (a sequential union-find in place of the atomics: the larger root goes
// under the smaller), the roots ranked, the closed forms per run, the weight sums per aligned 16-byte piece and the labels per aligned
// piece of four, each bisecting into its row's runs - so UBSan sees every product and sum the device forms, and ASan every index into
// the map (allocated to its last row's last byte, no slack) and into the workspace arrays (sized by wsi_region::layout).  Before the
// corpus it walks the piece arithmetic the map kernels share (csrc/map_dev.h) exhaustively; exit status 5 where that fails.
//   usage: regions_san CORPUS RESULTS
//   CORPUS : u32 cases, then per case i32 kind, W, H, connectivity, shift (bytes before the map's first byte), pitch, has_weight, n;
//            kind 0: 256 bytes of traced table, H x W map bytes, then H x W weight bytes where has_weight;
//            kind 1: n runs of three i32 (y, x0, x1), hand-made
//   RESULTS: kind 0: u32 n_runs, u32 n_regions, n_regions x 16 i64, H x W i32 labels; kind 1: n x 6 i64 (area sx sy sxx sxy syy)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../wsi_segmentation_pipeline_amd/csrc/regions_dev.h"

using namespace wsi_region;

static bool read_n(FILE* f, void* v, size_t bytes) { return bytes == 0 || fread(v, bytes, 1, f) == 1; }

static uint32_t find_root(const std::vector<uint32_t>& parent, uint32_t r) {
    while (parent.at(r) != r) r = parent.at(r);
    return r;
}

static int byte_at(const unsigned char* map, long long pitch, int W, int y, int x) { return x < 0 || x >= W ? -1 : (int)map[(long long)y * pitch + x]; }

// The shared piece arithmetic (csrc/map_dev.h), exhaustively over real addresses: a segment of every length 1 .. 48 at every offset of its
// first byte inside an aligned 16-byte piece, its shift taken from that address as the kernels take it.  The pieces 0 ..
// pieces_for(len) - 1 cover every byte of [0, len) exactly once and nothing outside it, and the address a whole piece is fetched from,
// seg + k0, is a multiple of 16.
static bool pieces_cover_every_segment() {
    alignas(16) static const unsigned char line[80] = {};
    for (int offset = 0; offset < 16; ++offset)
        for (int len = 1; len <= 48; ++len) {
            const unsigned char* seg = line + offset;
            const int shift = wsi_map::piece_shift(seg);
            if (shift != offset) return false;
            std::vector<int> seen((size_t)len, 0);
            for (int piece = 0; piece < wsi_map::pieces_for(len); ++piece) {
                const wsi_map::Piece p = wsi_map::piece_of(shift, piece, len);
                if (p.ke <= p.kb) continue;
                if (p.kb < 0 || p.ke > len || p.kb < p.k0 || p.ke > p.k0 + 16) return false;
                if (p.ke - p.kb == 16 && (uintptr_t)(seg + p.k0) % 16 != 0) return false;
                for (int k = p.kb; k < p.ke; ++k) ++seen.at((size_t)k);
            }
            for (int k = 0; k < len; ++k) if (seen.at((size_t)k) != 1) return false;
        }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CORPUS RESULTS\n", argv[0]); return 2; }
    if (!pieces_cover_every_segment()) { fprintf(stderr, "wsi_map::piece_of does not cover a segment exactly once\n"); return 5; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    unsigned cases = 0;
    if (!read_n(in, &cases, 4)) return 2;
    for (unsigned c = 0; c < cases; ++c) {
        int head[8];
        if (!read_n(in, head, sizeof head)) return 2;
        const int kind = head[0], W = head[1], H = head[2], conn = head[3], shift = head[4], has_weight = head[6], given = head[7];
        const long long pitch = head[5];
        if (kind == 1) {
            for (int k = 0; k < given; ++k) {
                int r[3];
                if (!read_n(in, r, sizeof r)) return 2;
                const Sums s = run_sums(r[0], r[1], r[2]);
                const long long v[6] = {s.area, s.sx, s.sy, s.sxx, s.sxy, s.syy};
                fwrite(v, 8, 6, out);
            }
            continue;
        }
        if (kind != 0 || W < 1 || H < 1 || W > LIMIT || H > LIMIT || shift < 0 || pitch < W || (conn != 4 && conn != 8)) return 2;
        const int d = conn == 8 ? 1 : 0;
        unsigned char table[256];
        if (!read_n(in, table, 256)) return 2;
        const Traced tr = wsi_map::traced_bits(table);
        const size_t bytes = (size_t)shift + (size_t)(H - 1) * pitch + W;
        unsigned char* buf = (unsigned char*)malloc(bytes);
        unsigned char* wbuf = has_weight ? (unsigned char*)malloc(bytes) : nullptr;
        memset(buf, 0xA5, bytes);
        const unsigned char* map = buf + shift;
        for (int y = 0; y < H; ++y) if (!read_n(in, buf + shift + y * pitch, W)) return 2;
        if (wbuf) {
            memset(wbuf, 0xA5, bytes);
            for (int y = 0; y < H; ++y) if (!read_n(in, wbuf + shift + y * pitch, W)) return 2;
        }
        const unsigned char* weight = wbuf ? wbuf + shift : nullptr;

        // count: starts per chunk, then the exclusive scan of the chunk sums
        const long long cpr = chunks_per_row(W), chunks = count_chunks(W, H);
        if (count_workspace_bytes(W, H) < 4 * ((size_t)chunks + 1)) return 3;
        std::vector<uint32_t> sums((size_t)chunks + 1);
        for (long long b = 0; b < chunks; ++b) {
            const int y = (int)(b / cpr), cx0 = (int)(b % cpr) * CHUNK, cw = W - cx0 < CHUNK ? W - cx0 : CHUNK;
            uint32_t count = 0;
            for (int i = 0; i < cw; ++i) count += starts_run(byte_at(map, pitch, W, y, cx0 + i - 1), byte_at(map, pitch, W, y, cx0 + i), tr);
            sums.at((size_t)b) = count;
        }
        uint32_t carry = 0;
        for (long long b = 0; b < chunks; ++b) { const uint32_t v = sums.at((size_t)b); sums.at((size_t)b) = carry; carry += v; }
        sums.at((size_t)chunks) = carry;
        const uint32_t n = carry;
        fwrite(&n, 4, 1, out);
        if (n == 0) {
            const uint32_t zero = 0;
            fwrite(&zero, 4, 1, out);
            const std::vector<int32_t> labels((size_t)W * H, 0);
            fwrite(labels.data(), 4, labels.size(), out);
            free(buf);
            free(wbuf);
            continue;
        }
        // the workspace, carved as the kernels carve it
        const Layout l = layout(H, n);
        if (l.row_first < l.runs + 16 * (size_t)n || l.bytes < l.sums + 4 * ((size_t)scan_chunks(n) + 1)) return 3;
        std::vector<Run> runs(n);
        std::vector<uint32_t> row_first((size_t)H + 1), parent(n), up(n), root(n), flag((size_t)n + 1), rank((size_t)n + 1), id(n);
        // runs: a start writes y, x0, cls, the run's end pixel writes x1 of the same record
        for (long long b = 0; b < chunks; ++b) {
            const int y = (int)(b / cpr), cx0 = (int)(b % cpr) * CHUNK, cw = W - cx0 < CHUNK ? W - cx0 : CHUNK;
            if (cx0 == 0) row_first.at(y) = sums.at((size_t)b);
            long long number = sums.at((size_t)b);
            for (int i = 0; i < cw; ++i) {
                const int left = byte_at(map, pitch, W, y, cx0 + i - 1), mid = byte_at(map, pitch, W, y, cx0 + i), right = byte_at(map, pitch, W, y, cx0 + i + 1);
                const bool st = starts_run(left, mid, tr), en = ends_run(mid, right, tr);
                number += st;
                if (st) {
                    Run& r = runs.at((size_t)(number - 1));
                    r.y = y; r.x0 = cx0 + i; r.cls = mid;
                    parent.at((size_t)(number - 1)) = (uint32_t)(number - 1);
                }
                if (en) runs.at((size_t)(number - 1)).x1 = cx0 + i + 1;
            }
        }
        row_first.at(H) = sums.at((size_t)chunks);
        // link
        for (uint32_t r = 0; r < n; ++r) {
            const Run me = runs[r];
            uint32_t shared_sides = 0;
            if (me.y > 0) {
                const uint32_t end = row_first.at(me.y);
                for (uint32_t a = first_ending_after(runs.data(), row_first.at(me.y - 1), end, me.x0 - d); a < end; ++a) {
                    const Run o = runs.at(a);
                    if (!(o.x0 < me.x1 + d)) break;
                    if (!joins(o.x0, o.x1, me.x0, me.x1, d)) return 4;      // the bisection and the walk's end are the join test
                    if (o.cls != me.cls) continue;
                    const uint32_t ra = find_root(parent, r), rb = find_root(parent, a);
                    if (ra != rb) parent.at(ra > rb ? ra : rb) = ra > rb ? rb : ra;
                    shared_sides += (uint32_t)overlap(o.x0, o.x1, me.x0, me.x1);
                }
            }
            up.at(r) = shared_sides;
        }
        // rank
        uint32_t n_regions = 0;
        for (uint32_t r = 0; r < n; ++r) {
            root.at(r) = find_root(parent, r);
            flag.at(r) = root[r] == r;
            rank.at(r) = n_regions;
            n_regions += flag[r];
        }
        rank.at(n) = n_regions;
        for (uint32_t r = 0; r < n; ++r) id.at(r) = rank.at(root[r]) + 1;
        // table
        std::vector<long long> tab((size_t)n_regions * RECORD_WORDS, 0);
        for (uint32_t k = 0; k < n_regions; ++k) tab.at((size_t)k * RECORD_WORDS + BOX_X0) = 0x7fffffffffffffffLL;
        for (uint32_t r = 0; r < n; ++r) {
            const Run me = runs[r];
            long long* rec = &tab.at((size_t)(id[r] - 1) * RECORD_WORDS);
            const Sums s = run_sums(me.y, me.x0, me.x1);
            rec[AREA] += s.area; rec[SX] += s.sx; rec[SY] += s.sy; rec[SXX] += s.sxx; rec[SXY] += s.sxy; rec[SYY] += s.syy;
            rec[PERIM] += run_perimeter(s.area, up[r]);
            if (me.x0 < rec[BOX_X0]) rec[BOX_X0] = me.x0;
            if (me.x1 > rec[BOX_X1]) rec[BOX_X1] = me.x1;
            if (me.y + 1 > rec[BOX_Y1]) rec[BOX_Y1] = me.y + 1;
            if (touches_border(me.y, me.x0, me.x1, W, H)) rec[BORDER] = 1;
            if (root[r] == r) { rec[BOX_Y0] = me.y; rec[FIRST] = (long long)me.y * W + me.x0; rec[CLS] = me.cls; }
        }
        if (weight) {
            const int pieces = wsi_map::pieces_for(W);
            for (int y = 0; y < H; ++y)
                for (int piece = 0; piece < pieces; ++piece) {
                    const unsigned char* seg = weight + (long long)y * pitch;
                    const wsi_map::Piece p = wsi_map::piece_of(wsi_map::piece_shift(seg), piece, W);
                    const int kb = p.kb, ke = p.ke;
                    if (ke <= kb) continue;
                    const uint32_t end = row_first.at(y + 1);
                    for (uint32_t r = first_ending_after(runs.data(), row_first.at(y), end, kb); r < end; ++r) {
                        const Run o = runs.at(r);
                        if (o.x0 >= ke) break;
                        const int a = o.x0 > kb ? o.x0 : kb, b = o.x1 < ke ? o.x1 : ke;
                        for (int k = a; k < b; ++k) tab.at((size_t)(id[r] - 1) * RECORD_WORDS + WSUM) += seg[k];
                    }
                }
        }
        // paint: rows of W labels exactly, pieces of four aligned to the row's own address
        std::vector<int32_t> labels((size_t)W * H, -1);
        const int pieces = (W + 3) / 4 + 1;
        for (int y = 0; y < H; ++y) {
            int32_t* row = labels.data() + (size_t)y * W;
            const int sh = (int)(((uintptr_t)row & 15u) >> 2);
            for (int piece = 0; piece < pieces; ++piece) {
                const int e0 = piece * 4 - sh, eb = e0 < 0 ? 0 : e0, ee = e0 + 4 < W ? e0 + 4 : W;
                if (ee <= eb) continue;
                const uint32_t end = row_first.at(y + 1);
                uint32_t r = first_ending_after(runs.data(), row_first.at(y), end, eb);
                for (int x = eb; x < ee; ++x) {
                    while (r < end && runs.at(r).x1 <= x) ++r;
                    labels.at((size_t)y * W + x) = r < end && runs.at(r).x0 <= x ? (int32_t)id.at(r) : 0;
                }
            }
        }
        fwrite(&n_regions, 4, 1, out);
        fwrite(tab.data(), 8, tab.size(), out);
        fwrite(labels.data(), 4, labels.size(), out);
        free(buf);
        free(wbuf);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
