// Stand-alone host program over the region hulls' shared arithmetic (csrc/region_hulls_dev.h: the source the kernels of
// region_hulls.hip compile).  tests/test_region_hulls_cpu.py builds it with the host compiler under -fsanitize=address,undefined and runs
// it over a corpus it wrote; it is never loaded into python.  It walks a region table the way the kernels' lanes do - the heights and
// their scan, min and max of the run corners per corner row, the first-level chains per segment of a piece of PIECE rows with the stack
// in the place of the rows read, the second-level chain of every region that crosses a piece border over its segments' survivors, the
// vertex of every slot (vertex_slot), one scan_hull per vertex and one pick_record per hull - so UBSan sees every product and sum the
// device forms, and ASan every index into the workspace arrays (sized by wsi_hull::layout, no slack).
//   usage: region_hulls_san CORPUS RESULTS
//   CORPUS : u32 cases, then per case i32 kind, n_runs, n_regions;
//            kind 0: n_runs x {y, x0, x1, id} i32, n_regions x {y0, y1} i32;
//            kind 1: n_runs x {n1, d1, n2, d2} u64: ratio_less at hand-made operands
//   RESULTS: kind 0: u32 V, n_regions x 16 i64, V x 2 i32; kind 1: n_runs x {u64 hi, u64 lo of n1 d2, u64 less}
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../wsi_segmentation_pipeline_amd/csrc/region_hulls_dev.h"

using namespace wsi_hull;

static bool read_n(FILE* f, void* v, size_t bytes) { return bytes == 0 || fread(v, bytes, 1, f) == 1; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CORPUS RESULTS\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    unsigned cases = 0;
    if (!read_n(in, &cases, 4)) return 2;
    for (unsigned c = 0; c < cases; ++c) {
        int head[3];
        if (!read_n(in, head, sizeof head)) return 2;
        const int kind = head[0];
        const long long n_runs = head[1], n = head[2];
        if (kind == 1) {
            for (long long k = 0; k < n_runs; ++k) {
                u64 v[4];
                if (!read_n(in, v, sizeof v)) return 2;
                const U128 p = mul_wide(v[0], v[3]);
                const u64 res[3] = {p.hi, p.lo, (u64)ratio_less(v[0], v[1], v[2], v[3])};
                fwrite(res, 8, 3, out);
            }
            continue;
        }
        if (kind != 0 || n_runs < 1 || n < 1 || n > n_runs) return 2;
        std::vector<int32_t> runs((size_t)n_runs * 4), box((size_t)n * 2);
        if (!read_n(in, runs.data(), runs.size() * 4) || !read_n(in, box.data(), box.size() * 4)) return 2;
        // the workspace, carved as the kernels carve it: every array exactly as large as the layout says
        const Layout l = layout(n_runs, n);
        const size_t rows = (size_t)max_rows(n_runs, n);
        if (l.row_off - l.height < 4 * ((size_t)n + 1) || l.hi - l.lo < 4 * rows || l.bytes - l.picks < 64 * rows) return 3;
        std::vector<uint32_t> height((size_t)n + 1), row_off((size_t)n + 1), st[2], seg[2], cnt[2], count((size_t)n + 1), first((size_t)n + 1);
        std::vector<int32_t> x[2];                              // side 0: hi, 1: lo
        for (int s = 0; s < 2; ++s) { st[s].assign(rows, 0); seg[s].assign(rows, 0); cnt[s].assign((size_t)n, 0); }
        x[0].assign(rows, INT_MIN);
        x[1].assign(rows, INT_MAX);
        // rows
        uint32_t total = 0;
        for (long long k = 0; k < n; ++k) {
            long long h = (long long)box.at(2 * k + 1) - box.at(2 * k) + 1;
            h = h < 2 ? 2 : (h > LIMIT + 1 ? LIMIT + 1 : h);
            height.at(k) = (uint32_t)h;
            row_off.at(k) = total;
            total += (uint32_t)h;
        }
        row_off.at(n) = total;
        if (total > rows) return 3;
        for (long long r = 0; r < n_runs; ++r) {
            const int32_t y = runs[4 * r], x0 = runs[4 * r + 1], x1 = runs[4 * r + 2], id = runs[4 * r + 3];
            if (id < 1 || id > n) return 2;
            const long long j = (long long)y - box.at(2 * (id - 1)), at = (long long)row_off.at(id - 1) + j;
            if (j < 0 || at + 1 >= (long long)row_off.at(id)) return 4;
            for (long long a = at; a <= at + 1; ++a) {
                if (x0 < x[1].at(a)) x[1].at(a) = x0;
                if (x1 > x[0].at(a)) x[0].at(a) = x1;
            }
        }
        // chains, first level: one lane per piece, its stack in the place of the rows it has read
        std::vector<uint32_t> stack(rows);
        for (long long g0 = 0; g0 < total; g0 += PIECE) {
            const long long end = g0 + PIECE < total ? g0 + PIECE : total;
            uint32_t k = owner_of(row_off.data(), (uint32_t)n, (uint32_t)g0);
            long long row = g0;
            while (row < end && k < n) {
                const long long s = row_off.at(k), e = row_off.at(k + 1), seg_end = e < end ? e : end;
                if (seg_end <= row) return 4;
                for (int side = 0; side < 2; ++side) {
                    long long sp = 0;
                    for (long long li = row; li < seg_end; ++li) {
                        while (sp >= 2) {
                            const long long b = stack.at(row + sp - 1), a = stack.at(row + sp - 2);
                            if (!pops(side, x[side].at(a), a, x[side].at(b), b, x[side].at(li), li)) break;
                            --sp;
                        }
                        stack.at(row + sp++) = (uint32_t)li;
                    }
                    for (long long i = 0; i < sp; ++i) st[side].at(row + i) = (uint32_t)(stack.at(row + i) - s);
                    seg[side].at(row) = (uint32_t)sp;
                    if (row == s && seg_end == e) cnt[side].at(k) = (uint32_t)sp;
                }
                if (row == s && seg_end == e) count.at(k) = cnt[0].at(k) + cnt[1].at(k);
                row = seg_end;
                if (row == e) ++k;
            }
        }
        // second level: one workgroup per piece border
        for (long long border = PIECE; border < total; border += PIECE) {
            const uint32_t k = owner_of(row_off.data(), (uint32_t)n, (uint32_t)(border - 1));
            const long long s = row_off.at(k), e = row_off.at(k + 1);
            if (e <= border || s < border - PIECE) continue;
            for (int side = 0; side < 2; ++side) {
                std::vector<long long> sx, sj;
                for (long long sg = s; sg < e; sg = (sg / PIECE + 1) * PIECE) {
                    const uint32_t got = seg[side].at(sg);
                    if (got > (sg / PIECE + 1) * PIECE - sg) return 4;
                    for (uint32_t i = 0; i < got; ++i) {
                        const long long j = st[side].at(sg + i), px = x[side].at(s + j);
                        while (sx.size() >= 2 && pops(side, sx[sx.size() - 2], sj[sj.size() - 2], sx.back(), sj.back(), px, j)) { sx.pop_back(); sj.pop_back(); }
                        if (sx.size() >= (size_t)STACK) return 6;
                        sx.push_back(px);
                        sj.push_back(j);
                    }
                }
                for (size_t i = 0; i < sj.size(); ++i) st[side].at(s + i) = (uint32_t)sj[i];
                cnt[side].at(k) = (uint32_t)sj.size();
            }
            count.at(k) = cnt[0].at(k) + cnt[1].at(k);
        }
        uint32_t V = 0;
        for (long long k = 0; k < n; ++k) { first.at(k) = V; V += count.at(k); }
        first.at(n) = V;
        if (V < 4 * n || V > 2 * rows) return 4;
        // emit: one lane per vertex
        std::vector<int32_t> vertices((size_t)V * 2);
        for (uint32_t v = 0; v < V; ++v) {
            const uint32_t k = owner_of(first.data(), (uint32_t)n, v), i = v - first.at(k);
            int side;
            uint32_t at;
            vertex_slot(i, cnt[0].at(k), cnt[1].at(k), &side, &at);
            const uint32_t j = st[side].at(row_off.at(k) + at);
            vertices.at(2 * v) = x[side].at(row_off.at(k) + j);
            vertices.at(2 * v + 1) = box.at(2 * k) + (int32_t)j;
        }
        // measure: one lane per vertex, then one per hull
        std::vector<Pick> picks(V);
        if (sizeof(Pick) != 32) return 3;
        for (uint32_t v = 0; v < V; ++v) {
            const uint32_t k = owner_of(first.data(), (uint32_t)n, v);
            picks.at(v) = scan_hull(vertices.data() + 2 * first.at(k), count.at(k), v - first.at(k));
        }
        std::vector<long long> table((size_t)n * RECORD_WORDS);
        for (long long k = 0; k < n; ++k)
            pick_record(vertices.data() + 2 * first.at(k), picks.data() + first.at(k), count.at(k), first.at(k), table.data() + k * RECORD_WORDS);
        fwrite(&V, 4, 1, out);
        fwrite(table.data(), 8, table.size(), out);
        fwrite(vertices.data(), 4, vertices.size(), out);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
