// Host side of the JPEG path: table parse and marker walk (include/wsi_hip.h, wsi_jpeg_parse_tables / wsi_jpeg_walk).  Plain C++, no
// GPU and no HIP header: jpeg.hip wraps these in the C-ABI entries, tests/jpeg_san_main.cpp runs them under the host sanitizers.
// Every read goes through Span, which holds [0, n) of one stream and answers out-of-range reads with `false`.
#pragma once
#include <string.h>
#include "jpeg_dev.h"

namespace wsi_jpeg {

struct Span {
    const unsigned char* p;
    size_t n;
    bool u8(size_t i, unsigned* v) const { if (i >= n) return false; *v = p[i]; return true; }
    bool u16(size_t i, unsigned* v) const { if (n < 2 || i > n - 2) return false; *v = ((unsigned)p[i] << 8) | p[i + 1]; return true; }
};

// derive the look-up form from the 16 counts and the symbols (Annex C of the standard; the limits are libjpeg's jdhuff.c)
inline bool huff_build(const unsigned char* counts, const unsigned char* vals, int nvals, bool is_dc, wsi_jpeg_huff* h) {
    memset(h, 0, sizeof(*h));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int c = counts[l - 1];
        if (c == 0) {
            h->maxcode[l] = -1;
        } else {
            if (code + c > (1 << l)) return false;             // more codes than the length holds
            h->valoffset[l] = k - code;
            for (int i = 0; i < c; ++i) {
                const int sym = vals[k + i];
                if (is_dc && sym > 15) return false;
                if (l <= WSI_JPEG_LOOK_BITS) {
                    const int first = (code + i) << (WSI_JPEG_LOOK_BITS - l);
                    for (int f = 0; f < (1 << (WSI_JPEG_LOOK_BITS - l)); ++f) h->look[first + f] = (uint16_t)((l << 8) | sym);
                }
            }
            k += c;
            code += c;
            h->maxcode[l] = code - 1;
        }
        code <<= 1;
    }
    if (k != nvals) return false;
    h->maxcode[0] = -1;
    h->maxcode[17] = 0x7fffffff;
    memcpy(h->huffval, vals, (size_t)nvals);
    return true;
}

// one DQT segment body [at, at + len) into t
inline bool parse_dqt(const Span& s, size_t at, size_t len, wsi_jpeg_tables* t) {
    size_t i = at;
    const size_t end = at + len;
    while (i < end) {
        unsigned pq;
        if (!s.u8(i, &pq)) return false;
        const unsigned prec = pq >> 4, id = pq & 15;
        if (id > 3 || prec > 1) return false;
        ++i;
        if (end - i < 64u * (prec + 1)) return false;
        for (int k = 0; k < 64; ++k) {
            unsigned v;
            if (prec) { if (!s.u16(i, &v)) return false; i += 2; }
            else { if (!s.u8(i, &v)) return false; i += 1; }
            if (v == 0) return false;
            t->qt[id][k] = (uint16_t)v;
        }
        t->qt_present[id] = 1;
    }
    return true;
}
inline bool parse_dht(const Span& s, size_t at, size_t len, wsi_jpeg_tables* t) {
    size_t i = at;
    const size_t end = at + len;
    while (i < end) {
        unsigned tc;
        if (!s.u8(i, &tc)) return false;
        const unsigned cls = tc >> 4, id = tc & 15;
        if (cls > 1 || id > 1) return false;                  // baseline: two tables per class
        ++i;
        if (end - i < 16) return false;
        unsigned char counts[16], vals[256];
        int total = 0;
        for (int k = 0; k < 16; ++k) { unsigned v; if (!s.u8(i + k, &v)) return false; counts[k] = (unsigned char)v; total += (int)v; }
        i += 16;
        if (total > 256 || end - i < (size_t)total) return false;
        for (int k = 0; k < total; ++k) { unsigned v; if (!s.u8(i + k, &v)) return false; vals[k] = (unsigned char)v; }
        i += (size_t)total;
        if (!huff_build(counts, vals, total, cls == 0, &t->huff[cls * 2 + id])) return false;
        t->huff_present[cls * 2 + id] = 1;
    }
    return true;
}

struct Frame {
    bool have_sof = false, have_sos = false, own_tables = false;
    unsigned width = 0, height = 0, ncomp = 0, restart = 0;
    unsigned id[3] = {0, 0, 0}, h[3] = {0, 0, 0}, v[3] = {0, 0, 0}, tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    size_t scan_off = 0, scan_len = 0;
};

// Walk one stream.  `tables` is overlaid by the stream's DQT / DHT.  stop_at_sos: a table blob, nothing but tables is asked for.
inline int walk_stream(const Span& s, wsi_jpeg_tables* tables, Frame* f, bool tables_only) {
    unsigned m;
    if (!s.u16(0, &m) || m != 0xFFD8) return WSI_JPEG_MALFORMED;
    size_t i = 2;
    for (;;) {
        unsigned b;
        if (!s.u8(i, &b)) return tables_only ? 0 : WSI_JPEG_MALFORMED;             // the end without EOI
        if (b != 0xFF) return WSI_JPEG_MALFORMED;
        unsigned mk = 0xFF;
        while (mk == 0xFF) {                                   // fill bytes
            ++i;
            if (!s.u8(i, &mk)) return WSI_JPEG_MALFORMED;
        }
        ++i;
        if (mk == 0xD9) return (tables_only || f->have_sos) ? 0 : WSI_JPEG_MALFORMED;
        if (mk == 0x00 || mk == 0x01 || (mk >= 0xD0 && mk <= 0xD8)) return WSI_JPEG_MALFORMED;
        unsigned len;
        if (!s.u16(i, &len) || len < 2 || s.n - i < len) return WSI_JPEG_MALFORMED;
        const size_t body = i + 2, blen = len - 2;
        if (f->have_sos) return WSI_JPEG_MULTISCAN;            // a segment after the first scan: more scans, or tables for them
        if (mk == 0xDB) {
            if (!parse_dqt(s, body, blen, tables)) return WSI_JPEG_MALFORMED;
            f->own_tables = true;
        } else if (mk == 0xC4) {
            if (!parse_dht(s, body, blen, tables)) return WSI_JPEG_MALFORMED;
            f->own_tables = true;
        } else if (mk == 0xDD) {
            if (blen != 2 || !s.u16(body, &f->restart)) return WSI_JPEG_MALFORMED;
        } else if (mk >= 0xC0 && mk <= 0xCF && mk != 0xC8 && mk != 0xCC) {         // a frame header (C4 and CC were taken above / are DAC)
            if (tables_only) return 0;
            if (mk == 0xC2) return WSI_JPEG_PROGRESSIVE;
            if (mk != 0xC0 && mk != 0xC1) return WSI_JPEG_ARITHMETIC;
            if (f->have_sof) return WSI_JPEG_MALFORMED;
            unsigned prec, nc;
            if (blen < 6 || !s.u8(body, &prec) || !s.u16(body + 1, &f->height) || !s.u16(body + 3, &f->width) || !s.u8(body + 5, &nc))
                return WSI_JPEG_MALFORMED;
            if (prec != 8) return WSI_JPEG_PRECISION;
            if (nc != 1 && nc != 3) return WSI_JPEG_COMPONENTS;
            if (blen != 6 + 3 * nc || f->width == 0 || f->height == 0) return WSI_JPEG_MALFORMED;
            for (unsigned c = 0; c < nc; ++c) {
                unsigned hv;
                if (!s.u8(body + 6 + 3 * c, &f->id[c]) || !s.u8(body + 7 + 3 * c, &hv) || !s.u8(body + 8 + 3 * c, &f->tq[c])) return WSI_JPEG_MALFORMED;
                f->h[c] = hv >> 4; f->v[c] = hv & 15;
                if (f->tq[c] > 3) return WSI_JPEG_MALFORMED;
            }
            f->ncomp = nc;
            if (nc == 1) {
                f->h[0] = f->v[0] = 1;                         // one component: the factors only scale the MCU, which is one block
            } else {
                const bool luma_ok = (f->h[0] == 1 && f->v[0] == 1) || (f->h[0] == 2 && f->v[0] == 1) || (f->h[0] == 2 && f->v[0] == 2);
                if (!luma_ok || f->h[1] != 1 || f->v[1] != 1 || f->h[2] != 1 || f->v[2] != 1) return WSI_JPEG_SAMPLING;
            }
            if (f->width > (unsigned)MAX_DIM || f->height > (unsigned)MAX_DIM) return WSI_JPEG_MALFORMED;
            f->have_sof = true;
        } else if (mk == 0xDA) {
            if (tables_only) return 0;
            if (!f->have_sof) return WSI_JPEG_MALFORMED;
            unsigned ns;
            if (blen < 1 || !s.u8(body, &ns)) return WSI_JPEG_MALFORMED;
            if (ns < 1 || ns > 4 || blen != 4 + 2 * ns) return WSI_JPEG_MALFORMED;
            if (ns != f->ncomp) return WSI_JPEG_MULTISCAN;
            for (unsigned c = 0; c < ns; ++c) {
                unsigned cid, tt;
                if (!s.u8(body + 1 + 2 * c, &cid) || !s.u8(body + 2 + 2 * c, &tt)) return WSI_JPEG_MALFORMED;
                if (cid != f->id[c]) return WSI_JPEG_MALFORMED;                   // components in frame order
                f->td[c] = tt >> 4; f->ta[c] = tt & 15;
                if (f->td[c] > 1 || f->ta[c] > 1) return WSI_JPEG_MALFORMED;
            }
            unsigned ss, se, ahal;
            if (!s.u8(body + 1 + 2 * ns, &ss) || !s.u8(body + 2 + 2 * ns, &se) || !s.u8(body + 3 + 2 * ns, &ahal)) return WSI_JPEG_MALFORMED;
            if (ss != 0 || se != 63 || ahal != 0) return WSI_JPEG_MALFORMED;
            f->have_sos = true;
            f->scan_off = body + blen;
            // the scan runs to the first marker that is neither a stuffed FF 00 nor RSTn
            size_t j = f->scan_off;
            for (;;) {
                const void* q = j < s.n ? memchr(s.p + j, 0xFF, s.n - j) : nullptr;
                if (!q) return WSI_JPEG_MALFORMED;             // no marker ends the scan: truncated
                j = (size_t)((const unsigned char*)q - s.p);
                unsigned nx;
                if (!s.u8(j + 1, &nx)) return WSI_JPEG_MALFORMED;
                if (nx == 0x00 || (nx >= 0xD0 && nx <= 0xD7)) { j += 2; continue; }
                break;
            }
            f->scan_len = j - f->scan_off;
            i = j;
            continue;
        }
        // APPn, COM, DAC, DNL and the rest: stepped over
        i = body + blen;
    }
}

inline int parse_tables(const unsigned char* blob, size_t len, wsi_jpeg_tables* out) {
    memset(out, 0, sizeof(*out));
    Frame f;
    const Span s{blob, len};
    return walk_stream(s, out, &f, true);
}

inline int walk(const unsigned char* buf, size_t buf_len, const unsigned long long* off, const unsigned int* len, int n,
                const wsi_jpeg_tables* base, wsi_jpeg_tables* sets, int cap, int* n_sets, wsi_jpeg_tile* out) {
    for (int i = 0; i < n; ++i)
        if (off[i] > buf_len || len[i] > buf_len - off[i]) return -22;
    wsi_jpeg_tables* scratch = new wsi_jpeg_tables;
    int last = -1;                                             // consecutive tiles mostly share a set: look there first
    for (int i = 0; i < n; ++i) {
        wsi_jpeg_tile& t = out[i];
        memset(&t, 0, sizeof(t));
        if (len[i] == 0) { t.status = WSI_JPEG_EMPTY; continue; }
        if (base) memcpy(scratch, base, sizeof(*scratch)); else memset(scratch, 0, sizeof(*scratch));
        Frame f;
        const Span s{buf + off[i], len[i]};
        int st = walk_stream(s, scratch, &f, false);
        if (st == 0 && !(f.have_sof && f.have_sos)) st = WSI_JPEG_MALFORMED;
        if (st == 0 && f.scan_len > 0xffffffffull) st = WSI_JPEG_MALFORMED;
        for (unsigned c = 0; st == 0 && c < f.ncomp; ++c)
            if (!scratch->qt_present[f.tq[c]] || !scratch->huff_present[f.td[c]] || !scratch->huff_present[2 + f.ta[c]]) st = WSI_JPEG_MALFORMED;
        if (st == 0) {
            int found = -1;
            if (last >= 0 && memcmp(&sets[last], scratch, sizeof(*scratch)) == 0) found = last;
            for (int k = 0; found < 0 && k < *n_sets; ++k)
                if (memcmp(&sets[k], scratch, sizeof(*scratch)) == 0) found = k;
            if (found < 0) {
                if (*n_sets >= cap) st = WSI_JPEG_TABLE_CAPACITY;
                else { found = (*n_sets)++; memcpy(&sets[found], scratch, sizeof(*scratch)); }
            }
            if (st == 0) { t.table_set = found; last = found; }
        }
        t.status = st;
        if (st) continue;
        t.scan_off = off[i] + f.scan_off;
        t.scan_len = (unsigned)f.scan_len;
        t.width = (unsigned short)f.width; t.height = (unsigned short)f.height;
        t.restart = (unsigned short)f.restart;
        t.ncomp = (unsigned char)f.ncomp;
        for (unsigned c = 0; c < f.ncomp; ++c) {
            t.h[c] = (unsigned char)f.h[c]; t.v[c] = (unsigned char)f.v[c]; t.tq[c] = (unsigned char)f.tq[c];
            t.td[c] = (unsigned char)f.td[c]; t.ta[c] = (unsigned char)f.ta[c];
        }
    }
    delete scratch;
    return 0;
}

}  // namespace wsi_jpeg
