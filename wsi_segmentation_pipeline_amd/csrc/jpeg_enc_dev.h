// The per-tile entropy encode of baseline JPEG (sequential DCT, Huffman with the standard Annex K tables, 8 bit, one interleaved
// scan), written once for the device kernels (jpeg_enc.hip) and for host programs (tests/jenc_san_main.cpp runs this source under
// the host sanitizers).  No HIP header is needed: WSI_HD expands to __host__ __device__ under hipcc and to nothing elsewhere.
//
// One loop, encode_tile, and two sinks: CountSink counts the scan's bytes (the size pass), StoreSink stores them (the write pass).
// Bounds, by construction:
//   - coefficients are read at (mcu * blocks_per_mcu + block) * 64 + k with mcu < mcux * mcuy, block < blocks_per_mcu, k < 64: inside
//     the tile's area
//   - StoreSink writes byte `pos` of its range only while pos < cap; a scan longer than the range it was given is cut, never spilled
//   - a table index is (run << 4) | size with run, size <= 15 into 256 entries; a coefficient no baseline code exists for (AC size
//     above 10, DC difference size above 11) finds a code of length 0 - the transform kernel cannot produce one
//   - every loop has a fixed trip count (MCUs, blocks, 16 words of a block), clears one bit of the block's non-zero map per turn, or
//     removes 8 bits or a run of 16 per turn
// Spec: tests/jpeg_enc_oracle.py (scan_bytes), itself held to libjpeg's bytes.
#pragma once
#include "../../include/wsi_hip.h"

#if defined(__HIPCC__)
#define WSI_HD __host__ __device__
#else
#define WSI_HD
#endif

namespace wsi_jenc {

constexpr int MAX_DIM = 4096;                                  // tile width and height a batch may have (the decoder's limit)

// natural (row-major) position -> zigzag position
WSI_HD inline int natural_zigzag(int k) {
    constexpr unsigned char NZ[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                      41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                      46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return NZ[k & 63];
}

// The batch's geometry.  A tile is mcux x mcuy whole MCUs of `bpm` blocks: hs * vs luma blocks row by row, then Cb, then Cr.
struct Geometry {
    int width, height, ncomp, hs, vs;
    int mcux, mcuy, bpm;
    long long coefs;                                           // int16 coefficients of a tile
    long long tile_bytes;                                      // their bytes rounded up to 256: the workspace of one tile
};
WSI_HD inline bool geometry_make(int width, int height, int ncomp, int hs, int vs, Geometry* g) {
    if (width < 16 || width > MAX_DIM || height < 16 || height > MAX_DIM || (width & 15) || (height & 15) || (ncomp != 1 && ncomp != 3)) return false;
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)) || (ncomp == 1 && hs * vs != 1)) return false;
    g->width = width; g->height = height; g->ncomp = ncomp; g->hs = hs; g->vs = vs;
    g->mcux = width / (8 * hs);
    g->mcuy = height / (8 * vs);
    g->bpm = ncomp == 3 ? hs * vs + 2 : 1;
    g->coefs = (long long)g->mcux * g->mcuy * g->bpm * 64;
    g->tile_bytes = (g->coefs * 2 + 255) / 256 * 256;
    return true;
}

// Annex K: code counts of length 1..16 and the symbols of DC luma, DC chroma, AC luma, AC chroma
struct StdHuff {
    unsigned char counts[4][16];
    unsigned char symbols[4][162];
    unsigned char n[4];
};
constexpr StdHuff STD_HUFF = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
     {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
     {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
     {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}},
    {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
     {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
     {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
      193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
      56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
      115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
      164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
      212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
     {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
      9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
      55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
      106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
      162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
      210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}},
    {12, 12, 162, 162}};

// The encode form of the four tables: entry [table][symbol] = (code length << 16) | code, 0 where the table has no such symbol.
struct EncTables {
    unsigned code[4][256];
};
constexpr EncTables make_enc_tables() {
    EncTables t = {};
    for (int i = 0; i < 4; ++i) {
        unsigned code = 0;
        int k = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int j = 0; j < STD_HUFF.counts[i][l - 1]; ++j) {
                t.code[i][STD_HUFF.symbols[i][k]] = ((unsigned)l << 16) | code;
                ++code;
                ++k;
            }
            code <<= 1;
        }
    }
    return t;
}

struct CountSink {
    unsigned long long pos = 0;
    WSI_HD void byte(unsigned) { ++pos; }
};
struct StoreSink {
    unsigned char* p;                                          // the tile's range [p, p + cap)
    unsigned long long cap;
    unsigned long long pos = 0;
    WSI_HD void byte(unsigned b) {
        if (pos < cap) p[pos] = (unsigned char)b;
        ++pos;
    }
};

// jchuff.c's bit buffer: MSB first, at most 7 bits stay between calls; every 0xFF byte is followed by 0x00
template <class Sink>
struct BitWriter {
    Sink sink;
    unsigned long long acc = 0;
    int nbits = 0;
    WSI_HD void put(unsigned code, int size) {                 // size <= 16, code < 2^size
        acc = (acc << size) | code;
        nbits += size;
        while (nbits >= 8) {
            const unsigned b = (unsigned)(acc >> (nbits - 8)) & 255u;
            sink.byte(b);
            if (b == 255u) sink.byte(0);
            nbits -= 8;
        }
    }
    WSI_HD void entry(unsigned e) { put(e & 0xffffu, (int)(e >> 16)); }
    WSI_HD void flush() {                                      // pad the last byte with 1-bits
        if (nbits) put((1u << (8 - nbits)) - 1u, 8 - nbits);
        acc = 0;
    }
};
WSI_HD inline int bit_length(unsigned v) {                     // 0 for 0, at most 15: the size of a value, the low half of a run / size symbol
    int n = 0;
    while (v && n < 15) { ++n; v >>= 1; }
    return n;
}
// a value v != 0 of size s as libjpeg sends it: v, or v - 1 + 2^s for a negative v
WSI_HD inline unsigned value_bits(int v, int s) { return (unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1u); }

// bit k = coefficient k of the block is not zero.  Sixteen 8-byte loads (a block is 128 bytes at an 8-byte aligned address; little endian)
// instead of 64 dependent 2-byte ones: at the qualities slides are written with, most coefficients are zero and are never looked at again.
WSI_HD inline unsigned long long nonzero_map(const short* blk) {
    unsigned long long map = 0;
    for (int j = 0; j < 16; ++j) {
        unsigned long long w;
        __builtin_memcpy(&w, blk + 4 * j, 8);
        const unsigned long long four = (unsigned long long)((w & 0xffffull) != 0) | (unsigned long long)((w & 0xffff0000ull) != 0) << 1 |
                                        (unsigned long long)((w & 0xffff00000000ull) != 0) << 2 | (unsigned long long)((w >> 48) != 0) << 3;
        map |= four << (4 * j);
    }
    return map;
}

// Encode one tile's quantised coefficients coef[0 .. g.coefs) - MCU by MCU, component by component, zigzag - into the sink; `tab` is
// make_enc_tables()'s result (in LDS on the device).  restart: MCUs per interval, 0: none.  Returns the scan's bytes (the sink's count).
template <class Sink>
WSI_HD inline unsigned long long encode_tile(const short* coef, const Geometry& g, int restart, const unsigned (*tab)[256], Sink sink) {
    BitWriter<Sink> bw;
    bw.sink = sink;
    int pred[3] = {0, 0, 0};
    const int luma_blocks = g.bpm == 1 ? 1 : g.bpm - 2;
    const long long mcus = (long long)g.mcux * g.mcuy;
    int until_restart = restart, next_rst = 0;
    for (long long m = 0; m < mcus; ++m) {
        if (restart) {
            if (until_restart == 0) {
                bw.flush();
                bw.sink.byte(0xFF);
                bw.sink.byte(0xD0u + (unsigned)next_rst);
                next_rst = (next_rst + 1) & 7;
                until_restart = restart;
                pred[0] = pred[1] = pred[2] = 0;
            }
            --until_restart;
        }
        for (int b = 0; b < g.bpm; ++b) {
            const int c = b < luma_blocks ? 0 : b - luma_blocks + 1;
            const unsigned* dc = tab[c ? 1 : 0];
            const unsigned* ac = tab[c ? 3 : 2];
            const short* blk = coef + (m * g.bpm + b) * 64;
            const int diff = (int)blk[0] - pred[c];
            pred[c] = blk[0];
            int s = bit_length((unsigned)(diff < 0 ? -diff : diff));
            bw.entry(dc[s]);
            if (s) bw.put(value_bits(diff, s), s);
            // the AC coefficients: only the non-zero ones are visited, the runs between them come from their positions
            unsigned long long left = nonzero_map(blk) & ~1ull;
            int prev = 0;
            while (left) {
                const int k = __builtin_ctzll(left);
                left &= left - 1;
                int run = k - prev - 1;
                prev = k;
                const int v = blk[k];
                while (run > 15) { bw.entry(ac[0xF0]); run -= 16; }
                s = bit_length((unsigned)(v < 0 ? -v : v));
                bw.entry(ac[(run << 4) | s]);
                bw.put(value_bits(v, s), s);
            }
            if (prev != 63) bw.entry(ac[0]);
        }
    }
    bw.flush();
    return bw.sink.pos;
}

}  // namespace wsi_jenc
