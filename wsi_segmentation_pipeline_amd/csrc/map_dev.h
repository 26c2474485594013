// What the kernels over resident u8 maps (contour.hip, edt.hip, regions.hip) share and a host program can run too: the table of traced
// labels and the arithmetic of the aligned 16-byte pieces a row segment is fetched in.  contour_dev.h and regions_dev.h include this, so
// their stand-alone sanitizer programs compile it (tests/regions_san_main.cpp walks the piece arithmetic exhaustively).  No HIP header is
// needed: WSI_HD expands to __host__ __device__ under hipcc and to nothing elsewhere.  The kernels' shared HIP code: map_kernels.h.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WSI_HD __host__ __device__
#else
#define WSI_HD
#endif

namespace wsi_map {

struct Traced { uint32_t bits[8]; };                           // bit l: label l is traced

WSI_HD inline bool traced(const Traced& t, int label) { return (t.bits[label >> 5] >> (label & 31)) & 1u; }

// the 256-entry u8 table of the C entries (non-zero: traced) packed into bits, on the host
inline Traced traced_bits(const uint8_t* traced256) {
    Traced tr{};
    for (int l = 0; l < 256; ++l) if (traced256[l]) tr.bits[l >> 5] |= 1u << (l & 31);
    return tr;
}

// A segment of len bytes is fetched in the aligned 16-byte pieces of memory it touches: a whole piece as one uint4, a ragged end byte by
// byte, so nothing outside the segment is read.  shift = piece_shift(the segment's first byte); piece p of pieces_for(len) starts k0
// bytes from the segment's first byte (negative in piece 0 where shift > 0) and holds the segment's bytes [kb, ke): whole iff
// ke - kb == 16, and then seg + k0 is 16-byte aligned; nothing iff ke <= kb.
struct Piece { int k0, kb, ke; };

WSI_HD inline int piece_shift(const void* first) { return (int)((uintptr_t)first & 15u); }

WSI_HD inline int pieces_for(int len) { return (len + 15) / 16 + 1; }

WSI_HD inline Piece piece_of(int shift, int piece, int len) {
    Piece p;
    p.k0 = piece * 16 - shift;
    p.kb = p.k0 < 0 ? 0 : p.k0;
    p.ke = p.k0 + 16 < len ? p.k0 + 16 : len;
    return p;
}

}  // namespace wsi_map
