// The per-tile entropy decode of baseline JPEG (sequential DCT, Huffman, 8 bit, one interleaved scan), written once for the device
// kernel (jpeg.hip) and for host programs (tests/jpeg_san_main.cpp runs this source under the host sanitizers).  No HIP header is
// needed: WSI_HD expands to __host__ __device__ under hipcc and to nothing elsewhere.
//
// Bounds, by construction:
//   - bytes are read through BitReader alone, which holds [pos, end) of the tile's scan and never forms an address outside it
//   - coefficients are written at comp_off[c] + block * 64 + k with block < blocks of the component and k < 64, inside the tile's area
//   - every loop has a fixed trip count (MCUs, blocks, 63 coefficients, 16 code lengths) or adds at least 8 bits / stops per turn
//   - bad data ends in a status word
// Against libjpeg the loop is stricter in one place: a run + size symbol whose run passes coefficient 63 is WSI_JPEG_COEF_OVERRUN here
// (libjpeg stores the value at coefficient 63 and goes on), as are data left over at a restart marker or at the end of the scan
// (WSI_JPEG_EXCESS) and a dequantised value outside int16 (WSI_JPEG_RANGE).  Such a tile goes to the host decoder, so the level's bytes
// stay libjpeg's.  tests/jpeg_oracle.py refuses the same streams.
#pragma once
#include "../../include/wsi_hip.h"

#if defined(__HIPCC__)
#define WSI_HD __host__ __device__
#else
#define WSI_HD
#endif

namespace wsi_jpeg {

constexpr int MAX_DIM = 4096;                                  // frame width and height a batch may have

// zigzag position -> natural (row-major) position
WSI_HD inline int zigzag_natural(int k) {
    constexpr unsigned char ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return ZZ[k & 63];
}

// The batch's geometry and what follows from it.  Component c has bw[c] x bh[c] blocks (whole MCUs) in raster order.
struct Geometry {
    int width, height, ncomp, hs, vs;
    int mcux, mcuy;                                            // MCUs per row, MCU rows
    int bw[3], bh[3];
    long long comp_off[3];                                     // int16 index of component c's first coefficient in the tile's area
    long long coefs;                                           // int16 coefficients of a tile
    long long plane_off[3];                                    // byte index of component c's plane (bw * 8 x bh * 8) in the tile's planes
    long long coef_bytes, plane_bytes;                         // a tile's coefficients and its planes, each rounded up to 256 bytes
    long long tile_bytes;                                      // their sum: the workspace of n tiles is n coefficient areas, then n plane areas
};
WSI_HD inline bool geometry_make(int width, int height, int ncomp, int hs, int vs, Geometry* g) {
    if (width < 1 || width > MAX_DIM || height < 1 || height > MAX_DIM || (ncomp != 1 && ncomp != 3)) return false;
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)) || (ncomp == 1 && hs * vs != 1)) return false;
    g->width = width; g->height = height; g->ncomp = ncomp; g->hs = hs; g->vs = vs;
    g->mcux = (width + 8 * hs - 1) / (8 * hs);
    g->mcuy = (height + 8 * vs - 1) / (8 * vs);
    long long co = 0, po = 0;
    for (int c = 0; c < 3; ++c) {
        const bool used = c < ncomp;
        g->bw[c] = used ? g->mcux * (c == 0 ? hs : 1) : 0;
        g->bh[c] = used ? g->mcuy * (c == 0 ? vs : 1) : 0;
        g->comp_off[c] = co;
        g->plane_off[c] = po;
        co += (long long)g->bw[c] * g->bh[c] * 64;
        po += (long long)g->bw[c] * g->bh[c] * 64;
    }
    g->coefs = co;
    g->coef_bytes = (co * 2 + 255) / 256 * 256;
    g->plane_bytes = (po + 255) / 256 * 256;
    g->tile_bytes = g->coef_bytes + g->plane_bytes;
    return true;
}
WSI_HD inline bool tile_matches(const wsi_jpeg_tile& t, const Geometry& g) {
    if (t.width != g.width || t.height != g.height || t.ncomp != g.ncomp) return false;
    for (int c = 0; c < g.ncomp; ++c)
        if (t.h[c] != (c == 0 ? g.hs : 1) || t.v[c] != (c == 0 ? g.vs : 1) || t.tq[c] > 3 || t.td[c] > 1 || t.ta[c] > 1) return false;
    return true;
}

// MSB-first bit buffer over [pos, end) of `p`.  The top `nbits` bits of `acc` are valid and the bits below them are zero.  fill()
// loads four bytes at once where four remain and none is 0xFF, single bytes otherwise (FF 00 -> FF; FF xx stops the reader in front
// of the marker).  After a stop nbits may go negative: the caller reads zeros and finds out from exhausted().
struct BitReader {
    const unsigned char* p;
    unsigned long long pos, end;
    unsigned long long acc;
    int nbits;
    int marker;                                                // 0, or the xx of the FF xx that stopped the reader
    bool stopped;

    WSI_HD void init(const unsigned char* base, unsigned long long begin, unsigned long long stop) {
        p = base; pos = begin; end = stop; acc = 0; nbits = 0; marker = 0; stopped = false;
    }
    WSI_HD void fill() {
        while (nbits <= 32 && !stopped) {
            if (pos + 4 <= end) {
                unsigned w;
                __builtin_memcpy(&w, p + pos, 4);              // one unaligned 4-byte load
                if ((((~w) - 0x01010101u) & w & 0x80808080u) == 0) {               // no byte of w is 0xFF
                    const unsigned be = __builtin_bswap32(w);
                    acc |= (unsigned long long)be << (32 - nbits);
                    nbits += 32;
                    pos += 4;
                    continue;
                }
            }
            if (pos >= end) { stopped = true; break; }
            const unsigned b = p[pos];
            if (b == 0xFF) {
                if (pos + 1 >= end) { stopped = true; marker = -1; break; }          // a lone FF at the end of the data
                const unsigned b2 = p[pos + 1];
                if (b2 != 0) { stopped = true; marker = (int)b2; break; }
                pos += 2;
            } else {
                pos += 1;
            }
            acc |= (unsigned long long)b << (56 - nbits);
            nbits += 8;
        }
    }
    WSI_HD unsigned peek(int n) const { return (unsigned)(acc >> (64 - n)); }        // 1 <= n <= 32
    WSI_HD void skip(int n) { acc <<= n; nbits -= n; }
    WSI_HD bool exhausted() const { return nbits < 0; }
    // byte-align, expect RSTn, step over it, restart the buffer
    WSI_HD int restart(int expect) {
        // whole unread bytes in the buffer mean the interval's data went on where the marker was due
        if (nbits >= 8) return WSI_JPEG_EXCESS;
        if (!stopped) { acc = 0; nbits = 0; fill(); if (nbits > 0 || !stopped) return WSI_JPEG_EXCESS; }
        if (marker != 0xD0 + (expect & 7)) return marker > 0 ? WSI_JPEG_SHORT : WSI_JPEG_EXHAUSTED;
        pos += 2;
        acc = 0; nbits = 0; marker = 0; stopped = false;
        return 0;
    }
    WSI_HD int status_at_stop() const { return marker != 0 ? WSI_JPEG_SHORT : WSI_JPEG_EXHAUSTED; }
};

// one Huffman symbol; -1: no code of up to 16 bits matches
WSI_HD inline int huff_decode(BitReader& br, const wsi_jpeg_huff* h) {
    const unsigned e = h->look[br.peek(WSI_JPEG_LOOK_BITS)];
    if (e != 0) {
        br.skip((int)(e >> 8));
        return (int)(e & 255u);
    }
    int l = WSI_JPEG_LOOK_BITS + 1;
    int code = (int)br.peek(l);
    while (l <= 16 && code > h->maxcode[l]) {
        ++l;
        if (l <= 16) code = (int)br.peek(l);
    }
    if (l > 16) return -1;
    br.skip(l);
    return h->huffval[(code + h->valoffset[l]) & 255];
}
WSI_HD inline int receive_extend(BitReader& br, int s) {       // 1 <= s <= 15
    const int r = (int)br.peek(s);
    br.skip(s);
    return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
}

// Decode one tile's scan into coef[0 .. g.coefs): dequantised, natural order, only non-zero values are written (the area is zero
// beforehand).  `bytes` holds the scan at [t.scan_off, t.scan_off + t.scan_len); the caller has checked that range against its buffer
// and t against g (tile_matches).  Returns 0 or a WSI_JPEG_* status.
WSI_HD inline int decode_tile(const unsigned char* bytes, const wsi_jpeg_tile& t, const wsi_jpeg_tables* tab, const Geometry& g, short* coef) {
    BitReader br;
    br.init(bytes, t.scan_off, t.scan_off + t.scan_len);
    int pred[3] = {0, 0, 0};
    const int restart = t.restart;
    int until_restart = restart, next_rst = 0;
    for (int my = 0; my < g.mcuy; ++my) {
        for (int mx = 0; mx < g.mcux; ++mx) {
            if (restart) {
                if (until_restart == 0) {
                    const int rc = br.restart(next_rst);
                    if (rc) return rc;
                    next_rst = (next_rst + 1) & 7;
                    until_restart = restart;
                    pred[0] = pred[1] = pred[2] = 0;
                }
                --until_restart;
            }
            for (int c = 0; c < g.ncomp; ++c) {
                const int ch = c == 0 ? g.hs : 1, cv = c == 0 ? g.vs : 1;
                const unsigned short* q = tab->qt[t.tq[c] & 3];
                const wsi_jpeg_huff* hdc = &tab->huff[t.td[c] & 1];
                const wsi_jpeg_huff* hac = &tab->huff[2 + (t.ta[c] & 1)];
                for (int by = 0; by < cv; ++by) {
                    for (int bx = 0; bx < ch; ++bx) {
                        const long long block = (long long)(my * cv + by) * g.bw[c] + (mx * ch + bx);      // < bw * bh
                        short* out = coef + g.comp_off[c] + block * 64;
                        br.fill();
                        int s = huff_decode(br, hdc);
                        if (s < 0 || s > 15) return br.exhausted() ? br.status_at_stop() : WSI_JPEG_BAD_CODE;
                        if (s) {
                            br.fill();
                            pred[c] += receive_extend(br, s);
                        }
                        if (br.exhausted()) return br.status_at_stop();
                        {
                            const long long v = (long long)pred[c] * (long long)q[0];           // |pred| < 2^17, q < 2^16
                            if (pred[c] < -32768 || pred[c] > 32767 || v < -32768 || v > 32767) return WSI_JPEG_RANGE;
                            if (v) out[0] = (short)v;
                        }
                        int k = 1;
                        for (int turn = 0; turn < 63 && k < 64; ++turn) {
                            br.fill();
                            const int rs = huff_decode(br, hac);
                            if (rs < 0) return br.exhausted() ? br.status_at_stop() : WSI_JPEG_BAD_CODE;
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) { k = 64; break; }                    // end of block
                                k += 16;                                           // ZRL; one that passes 63 ends the block, as in libjpeg
                                continue;
                            }
                            k += r;
                            if (k > 63) return br.exhausted() ? br.status_at_stop() : WSI_JPEG_COEF_OVERRUN;
                            const long long v = (long long)receive_extend(br, s) * (long long)q[k];
                            if (br.exhausted()) return br.status_at_stop();
                            if (v < -32768 || v > 32767) return WSI_JPEG_RANGE;
                            out[zigzag_natural(k)] = (short)v;
                            ++k;
                        }
                        if (br.exhausted()) return br.status_at_stop();
                    }
                }
            }
        }
    }
    // the scan must end here: at most the padding bits of the last byte are left
    if (br.nbits >= 8) return WSI_JPEG_EXCESS;
    if (!br.stopped) { br.acc = 0; br.nbits = 0; br.fill(); if (br.nbits > 0) return WSI_JPEG_EXCESS; }
    if (br.marker != 0) return WSI_JPEG_EXCESS;                // a marker inside the scan range after the last MCU
    return 0;
}

}  // namespace wsi_jpeg
