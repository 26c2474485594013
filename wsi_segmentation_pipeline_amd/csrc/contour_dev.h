// The per-edge rule of the boundary tracer, written once for the device kernels (contour.hip) and for host programs
// (tests/contour_san_main.cpp runs this source under the host sanitizers).  No HIP header is needed: WSI_HD expands to
// __host__ __device__ under hipcc and to nothing elsewhere.  Spec: tests/contours_oracle.py.
//
// Pixel (x, y) is the corner square (x, y) - (x + 1, y + 1), x right, y down; side d of a pixel is 0 top (heading east), 1 right (south),
// 2 bottom (west), 3 left (north).  Everything the rule asks about an edge is answered by the four pixels round one corner, the Quad
// {NW, SW, SE, NE} (-1 outside the map): that order turns with the heading, so for heading d the pixel behind on the walk's side is
// q[(1 - d) & 3], the pixel ahead q[(2 - d) & 3] and the pixel ahead across the side q[(3 - d) & 3].
//   an edge LEAVES corner c with heading d iff its pixel q[(2 - d) & 3] is traced and the pixel across, q[(3 - d) & 3], differs;
//   an edge ARRIVING at c with heading d (its pixel P = q[(1 - d) & 3]) goes on with F = q[(2 - d) & 3] differing: right, d + 1;
//     else A = q[(3 - d) & 3] differing: straight, d; else left, d - 1 (F first: 4-connected foreground, loops never cross);
//   the tail of a leaving edge is a vertex unless the edge that arrives before it has the same heading: q[(1 - d) & 3] equals the
//     edge's pixel and q[(0 - d) & 3] differs from it.
// An edge's key is corner * 4 + d with corner = ty (W + 1) + tx of its tail; 1 <= W, H and H W <= 2^28 keep every key below 2^32.
#pragma once
#include <stdint.h>
#include "map_dev.h"

namespace wsi_contour {

using wsi_map::Traced;                                         // bit l: label l is traced
using wsi_map::traced;

constexpr int LIMIT = 1 << 29;                                 // every produced coordinate lies in [-LIMIT, LIMIT]
constexpr long long MAX_PIXELS = 1LL << 28;

struct Quad { int q[4]; };                                     // NW, SW, SE, NE; -1 outside the map

// the label of pixel (x, y), -1 outside the W x H map: no byte outside the H row segments is read
WSI_HD inline int label_at(const uint8_t* map, long long pitch, int W, int H, long long x, long long y) {
    return x < 0 || y < 0 || x >= W || y >= H ? -1 : (int)map[y * pitch + x];
}

WSI_HD inline Quad quad_at(const uint8_t* map, long long pitch, int W, int H, long long tx, long long ty) {
    Quad r;
    r.q[0] = label_at(map, pitch, W, H, tx - 1, ty - 1);
    r.q[1] = label_at(map, pitch, W, H, tx - 1, ty);
    r.q[2] = label_at(map, pitch, W, H, tx, ty);
    r.q[3] = label_at(map, pitch, W, H, tx, ty - 1);
    return r;
}

WSI_HD inline bool leaves(const Quad& c, int d, const Traced& t) {
    const int px = c.q[(2 - d) & 3];
    return px >= 0 && traced(t, px) && c.q[(3 - d) & 3] != px;
}

// bit d: an edge leaves this corner with heading d
WSI_HD inline unsigned leaving_mask(const Quad& c, const Traced& t) {
    unsigned m = 0;
    for (int d = 0; d < 4; ++d) m |= (unsigned)leaves(c, d, t) << d;
    return m;
}

// the heading on which the edge that arrives at this corner with heading d goes on
WSI_HD inline int next_heading(const Quad& c, int d) {
    const int p = c.q[(1 - d) & 3];
    if (c.q[(2 - d) & 3] != p) return (d + 1) & 3;
    if (c.q[(3 - d) & 3] != p) return d;
    return (d + 3) & 3;
}

WSI_HD inline bool tail_is_vertex(const Quad& c, int d) {
    const int px = c.q[(2 - d) & 3];
    return !(c.q[(1 - d) & 3] == px && c.q[(0 - d) & 3] != px);
}

WSI_HD inline int edge_label(const Quad& tail, int d) { return tail.q[(2 - d) & 3]; }

// the corner an edge of heading d ends at, as an index into the (W + 1)-wide corner grid
WSI_HD inline long long head_corner(long long corner, int d, int W) {
    return corner + (d == 0 ? 1 : d == 1 ? (long long)W + 1 : d == 2 ? -1 : -((long long)W + 1));
}

// x_tail y_head - x_head y_tail of the unit edge: the loop's sum is its area2 (collinear corners add nothing to a shoelace sum)
WSI_HD inline long long cross_term(long long tx, long long ty, int d) { return d == 0 ? -ty : d == 1 ? tx : d == 2 ? ty : -tx; }

// map corner -> level-0 coordinate along one axis; hi > 0 clamps to [0, hi - 1]
WSI_HD inline int level0(long long c, int origin, int step, int hi) {
    long long v = (long long)origin + c * step - step / 2;
    if (hi > 0) v = v < 0 ? 0 : v > (long long)hi - 1 ? (long long)hi - 1 : v;
    return (int)v;
}

}  // namespace wsi_contour
