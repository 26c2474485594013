// Baseline JPEG tiles of a pyramid level -> the resident (H, W, 3) u8 level (include/wsi_hip.h, wsi_jpeg_*).  Integer arithmetic
// throughout, libjpeg's default decode path restated (spec: tests/jpeg_oracle.py): the bytes equal libjpeg's.
//   entropy_kernel : one lane per tile runs jpeg_dev.h's decode_tile (the same source the host sanitizer program runs); a workgroup is
//                    one wave with `lanes` of its 64 lanes at work, so that a small batch still spreads over the chip and a wave
//                    serialises few divergent lanes.  The level's common table set sits in LDS, other sets are read from memory.
//   idct_kernel    : one lane per 8x8 block, jidctint's islow IDCT, eight 16-byte loads in, eight 8-byte stores out into u8 planes
//   store_kernel   : one lane per 16-byte-aligned 16-byte piece of one row of one tile in the level: "fancy" upsampling of the chroma
//                    planes, jdcolor's fixed-point YCbCr -> RGB, one 16-byte store, or bytes where the piece is cut by the row segment's ends
// The workspace of n tiles: n coefficient areas (zeroed by wsi_jpeg_entropy; the lane writes the non-zero coefficients), then n plane areas.
#include "internal.h"
#include "jpeg_walk.h"

namespace {
using wsi_jpeg::Geometry;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

__global__ __launch_bounds__(64) void entropy_kernel(const uint8_t* bytes, unsigned long long nbytes, const wsi_jpeg_tile* tiles, int n,
                                                     const wsi_jpeg_tables* sets, int n_sets, int common_set, Geometry g, uint8_t* ws,
                                                     int* status, int lanes) {
    __shared__ wsi_jpeg_tables common;
    {
        const unsigned* src = (const unsigned*)(sets + common_set);
        unsigned* dst = (unsigned*)&common;
        for (int k = threadIdx.x; k < (int)(sizeof(wsi_jpeg_tables) / 4); k += 64) dst[k] = src[k];
    }
    __syncthreads();
    if ((int)threadIdx.x >= lanes) return;
    const long long i = (long long)blockIdx.x * lanes + threadIdx.x;
    if (i >= n) return;
    const wsi_jpeg_tile t = tiles[i];
    int st = t.status;
    if (st == 0 && !wsi_jpeg::tile_matches(t, g)) st = WSI_JPEG_GEOMETRY;
    if (st == 0 && (t.scan_off > nbytes || t.scan_len > nbytes - t.scan_off || t.table_set < 0 || t.table_set >= n_sets)) st = WSI_JPEG_MALFORMED;
    if (st == 0) {
        const wsi_jpeg_tables* tab = t.table_set == common_set ? &common : sets + t.table_set;
        st = wsi_jpeg::decode_tile(bytes, t, tab, g, (short*)(ws + (size_t)i * (size_t)g.coef_bytes));
    }
    status[i] = st;
}

// jidctint.c, jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2, the multipliers FIX(x) = round(x * 2^13); 64-bit sums as libjpeg's JLONG
#define F_0_298631336 2446LL
#define F_0_390180644 3196LL
#define F_0_541196100 4433LL
#define F_0_765366865 6270LL
#define F_0_899976223 7373LL
#define F_1_175875602 9633LL
#define F_1_501321110 12299LL
#define F_1_847759065 15137LL
#define F_1_961570560 16069LL
#define F_2_053119869 16819LL
#define F_2_562915447 20995LL
#define F_3_072711026 25172LL

// one 1-D pass over x[0..7] (stride 1 in registers); SHIFT = the descale of this pass
template <int SHIFT>
__device__ inline void idct_1d(const int (&x)[8], int (&o)[8]) {
    long long z2 = x[2], z3 = x[6];
    long long z1 = (z2 + z3) * F_0_541196100;
    long long tmp2 = z1 + z3 * (-F_1_847759065);
    long long tmp3 = z1 + z2 * F_0_765366865;
    long long tmp0 = ((long long)x[0] + x[4]) * 8192;
    long long tmp1 = ((long long)x[0] - x[4]) * 8192;
    const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = x[7]; tmp1 = x[5]; tmp2 = x[3]; tmp3 = x[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    long long z4 = tmp1 + tmp3;
    const long long z5 = (z3 + z4) * F_1_175875602;
    tmp0 *= F_0_298631336; tmp1 *= F_2_053119869; tmp2 *= F_3_072711026; tmp3 *= F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    constexpr long long R = 1LL << (SHIFT - 1);
    o[0] = (int)((tmp10 + tmp3 + R) >> SHIFT); o[7] = (int)((tmp10 - tmp3 + R) >> SHIFT);
    o[1] = (int)((tmp11 + tmp2 + R) >> SHIFT); o[6] = (int)((tmp11 - tmp2 + R) >> SHIFT);
    o[2] = (int)((tmp12 + tmp1 + R) >> SHIFT); o[5] = (int)((tmp12 - tmp1 + R) >> SHIFT);
    o[3] = (int)((tmp13 + tmp0 + R) >> SHIFT); o[4] = (int)((tmp13 - tmp0 + R) >> SHIFT);
}
// libjpeg's range_limit[(x) & RANGE_MASK] after the IDCT: x + 128 clamped to 0..255, x taken modulo 1024 into [-512, 512)
__device__ inline unsigned range_limit(int x) {
    int v = (int)(x & 1023);
    v = v < 512 ? v : v - 1024;
    v += 128;
    return (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void idct_kernel(uint8_t* ws, const int* status, int n, Geometry g) {
    const long long blocks = g.coefs / 64;
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= blocks * n) return;
    const long long tile = id / blocks;
    long long b = id - tile * blocks;
    if (status[tile] != 0) return;
    int c = 0;
    if (g.ncomp == 3) {
        const long long b1 = g.comp_off[1] / 64, b2 = g.comp_off[2] / 64;
        c = b >= b2 ? 2 : b >= b1 ? 1 : 0;
        b -= g.comp_off[c] / 64;
    }
    const int bw = g.bw[c];
    const int by = (int)(b / bw), bx = (int)(b - (long long)by * bw);
    const s16x8* in = (const s16x8*)(ws + (size_t)tile * (size_t)g.coef_bytes) + (g.comp_off[c] / 8 + b * 8);
    int m[8][8];                                              // |pass 1 output| < 2^21 for int16 input
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const s16x8 v = in[r];
#pragma unroll
        for (int k = 0; k < 8; ++k) m[r][k] = v[k];
    }
    // pass 1: columns, descaled by CONST_BITS - PASS1_BITS
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int x[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = m[r][k];
        idct_1d<11>(x, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) m[r][k] = o[r];
    }
    // pass 2: rows, descaled by CONST_BITS + PASS1_BITS + 3
    uint8_t* plane = ws + (size_t)n * (size_t)g.coef_bytes + (size_t)tile * (size_t)g.plane_bytes + g.plane_off[c];
    const size_t pw = (size_t)bw * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        int o[8];
        idct_1d<18>(m[r], o);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { lo |= range_limit(o[k]) << (8 * k); hi |= range_limit(o[4 + k]) << (8 * k); }
        *(u32x2*)(plane + ((size_t)by * 8 + r) * pw + (size_t)bx * 8) = u32x2{lo, hi};
    }
}

struct StoreArgs {
    const uint8_t* planes;          // the first tile's planes
    const int* status;
    const int* tile_index;
    int transform, grid_cols, grid_rows;
    uint8_t* level;
    long long pitch;
    int H, W;
    int pieces_per_row;             // (width * 3 + 15) / 16 + 1: the aligned 16-byte pieces a row segment can touch
};

// chroma sample (x, y) of the full-size image from a plane of `pw` bytes per row with cw x chh real samples; jdsample.c's fancy
// upsampling, or replication where libjpeg uses it (cw <= 2)
__device__ inline int chroma_at(const uint8_t* p, int pw, int cw, int chh, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(size_t)y * pw + x];
    const int i = x >> 1, odd = x & 1;
    if (vs == 1) {
        const uint8_t* row = p + (size_t)y * pw;
        const int cur = row[i];
        if (cw <= 2) return cur;
        if (!odd) return i == 0 ? cur : (3 * cur + row[i - 1] + 1) >> 2;
        return i == cw - 1 ? cur : (3 * cur + row[i + 1] + 2) >> 2;
    }
    const int r = y >> 1;
    if (cw <= 2) return p[(size_t)r * pw + i];
    int far = (y & 1) ? r + 1 : r - 1;
    far = far < 0 ? 0 : far > chh - 1 ? chh - 1 : far;
    const uint8_t* r0 = p + (size_t)r * pw;
    const uint8_t* r1 = p + (size_t)far * pw;
    const int cur = 3 * r0[i] + r1[i];
    if (!odd) return i == 0 ? (cur * 4 + 8) >> 4 : (cur * 3 + (3 * r0[i - 1] + r1[i - 1]) + 8) >> 4;
    return i == cw - 1 ? (cur * 4 + 7) >> 4 : (cur * 3 + (3 * r0[i + 1] + r1[i + 1]) + 7) >> 4;
}
__device__ inline int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

__global__ __launch_bounds__(256) void store_kernel(StoreArgs a, Geometry g, int tile0) {
    const int tile = tile0 + blockIdx.y;
    if (a.status[tile] != 0) return;
    const int cell = a.tile_index[tile];
    if (cell < 0 || cell >= a.grid_cols * a.grid_rows) return;
    const long long x0 = (long long)(cell % a.grid_cols) * g.width, y0 = (long long)(cell / a.grid_cols) * g.height;
    if (x0 >= a.W || y0 >= a.H) return;
    const int vis_w = (int)(a.W - x0 < g.width ? a.W - x0 : g.width), vis_h = (int)(a.H - y0 < g.height ? a.H - y0 : g.height);
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int row = (int)(idx / a.pieces_per_row), piece = (int)(idx - (long long)row * a.pieces_per_row);
    if (row >= vis_h) return;
    uint8_t* seg = a.level + (y0 + row) * a.pitch + x0 * 3;                          // the row segment [seg, seg + 3 vis_w)
    const long long seg_len = 3LL * vis_w;
    const long long first = -(long long)((uintptr_t)seg & 15u) + 16LL * piece;       // the piece's first byte, relative to seg
    if (first >= seg_len) return;
    const long long lo = first < 0 ? 0 : first, hi = first + 16 < seg_len ? first + 16 : seg_len;      // its bytes inside the segment
    const uint8_t* planes = a.planes + (size_t)tile * (size_t)g.plane_bytes;
    const uint8_t* p0 = planes + g.plane_off[0];
    const int pw0 = g.bw[0] * 8;
    const uint8_t* p1 = planes + g.plane_off[1];
    const uint8_t* p2 = planes + g.plane_off[2];
    const int pwc = g.bw[1] * 8;
    const int cw = (g.width + g.hs - 1) / g.hs, chh = (g.height + g.vs - 1) / g.vs;
    unsigned long long w0 = 0, w1 = 0;                                               // the piece's 16 bytes
    const int px0 = (int)(lo / 3);
#pragma unroll
    for (int k = 0; k < 7; ++k) {                                                    // 16 bytes touch at most 7 pixels
        const int x = px0 + k;
        if (3LL * x >= hi) break;
        const int Y = p0[(size_t)row * pw0 + x];
        int c[3] = {Y, Y, Y};
        if (g.ncomp == 3) {
            const int u = chroma_at(p1, pwc, cw, chh, g.hs, g.vs, x, row), v = chroma_at(p2, pwc, cw, chh, g.hs, g.vs, x, row);
            if (a.transform) {                                                       // jdcolor.c build_ycc_rgb_table, 16 fractional bits
                const int cb = u - 128, cr = v - 128;
                c[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
                c[1] = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
                c[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
            } else {
                c[1] = u; c[2] = v;
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const long long at = 3LL * x + ch - first;                               // byte of the piece
            if (at >= 0 && at < 8) w0 |= (unsigned long long)c[ch] << (8 * at);
            else if (at >= 8 && at < 16) w1 |= (unsigned long long)c[ch] << (8 * (at - 8));
        }
    }
    if (lo == first && hi == first + 16) {
        *(u32x4*)(seg + first) = u32x4{(unsigned)w0, (unsigned)(w0 >> 32), (unsigned)w1, (unsigned)(w1 >> 32)};
    } else {
        for (long long j = lo; j < hi; ++j) {
            const int at = (int)(j - first);
            seg[j] = (uint8_t)((at < 8 ? w0 >> (8 * at) : w1 >> (8 * (at - 8))) & 255u);
        }
    }
}

int launched() { return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT; }

}  // namespace

// compute units of the current device (256 where it cannot be asked)
static int compute_units() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 256;
        cus = v;
    }
    return cus;
}
// lanes per wave of a one-lane-per-tile entropy kernel over n tiles (0 = this rule): at least four waves per compute unit where the
// batch has the tiles for it, and as few lanes per wave as that allows
int wsi_entropy_lanes(int n, int lanes) {
    if (lanes != 0) return lanes;
    const int waves = compute_units() * 4;
    lanes = (n + waves - 1) / waves;
    return lanes < 1 ? 1 : lanes > 64 ? 64 : lanes;
}

size_t wsi_jpeg_tables_bytes(void) { return sizeof(wsi_jpeg_tables); }
size_t wsi_jpeg_tile_bytes(void) { return sizeof(wsi_jpeg_tile); }

int wsi_jpeg_parse_tables(const uint8_t* blob, size_t len, wsi_jpeg_tables* out) {
    if (!blob || !out) return WSI_EINVAL;
    return wsi_jpeg::parse_tables(blob, len, out);
}

int wsi_jpeg_walk(const uint8_t* buf, size_t buf_len, const unsigned long long* off, const unsigned int* len, int n,
                  const wsi_jpeg_tables* base, wsi_jpeg_tables* sets, int cap, int* n_sets, wsi_jpeg_tile* tiles_out) {
    if (!buf || !off || !len || !sets || !n_sets || !tiles_out || n <= 0 || cap <= 0 || *n_sets < 0 || *n_sets > cap) return WSI_EINVAL;
    return wsi_jpeg::walk(buf, buf_len, off, len, n, base, sets, cap, n_sets, tiles_out);
}

size_t wsi_jpeg_workspace_bytes(int width, int height, int ncomp, int hs, int vs) {
    Geometry g;
    return wsi_jpeg::geometry_make(width, height, ncomp, hs, vs, &g) ? (size_t)g.tile_bytes : 0;
}

int wsi_jpeg_entropy(const uint8_t* bytes, size_t nbytes, const wsi_jpeg_tile* tiles, int n, const wsi_jpeg_tables* sets, int n_sets,
                     int common_set, int width, int height, int ncomp, int hs, int vs, void* ws, size_t ws_bytes, int* status, int lanes, void* stream) {
    Geometry g;
    if (!bytes || !tiles || !sets || !ws || !status || n <= 0 || n_sets <= 0 || common_set < 0 || common_set >= n_sets || lanes < 0 || lanes > 64) return WSI_EINVAL;
    if (!wsi_jpeg::geometry_make(width, height, ncomp, hs, vs, &g) || ((uintptr_t)ws & 15u) || ws_bytes / (size_t)g.tile_bytes < (size_t)n) return WSI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, (size_t)n * (size_t)g.coef_bytes, st) != hipSuccess) return WSI_EFAULT;
    lanes = wsi_entropy_lanes(n, lanes);
    hipLaunchKernelGGL(entropy_kernel, dim3((unsigned)((n + lanes - 1) / lanes)), dim3(64), 0, st, bytes, (unsigned long long)nbytes, tiles, n, sets,
                       n_sets, common_set, g, (uint8_t*)ws, status, lanes);
    return launched();
}

int wsi_jpeg_reconstruct(void* ws, size_t ws_bytes, const int* status, const int* tile_index, int n, int width, int height, int ncomp,
                         int hs, int vs, int transform, int grid_cols, int grid_rows, uint8_t* level, long long pitch, int H, int W,
                         void* stream) {
    Geometry g;
    if (!ws || !status || !tile_index || !level || n <= 0 || H <= 0 || W <= 0 || grid_cols <= 0 || grid_rows <= 0) return WSI_EINVAL;
    if (!wsi_jpeg::geometry_make(width, height, ncomp, hs, vs, &g) || ((uintptr_t)ws & 15u) || ws_bytes / (size_t)g.tile_bytes < (size_t)n) return WSI_EINVAL;
    if (pitch < 3LL * W || (transform != 0 && transform != 1)) return WSI_EINVAL;
    if ((long long)(grid_cols - 1) * width >= W || (long long)(grid_rows - 1) * height >= H) return WSI_EINVAL;
    if ((long long)grid_cols * grid_rows > 0x7fffffffLL) return WSI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const long long blocks = g.coefs / 64 * n;
    hipLaunchKernelGGL(idct_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st, (uint8_t*)ws, status, n, g);
    StoreArgs a;
    a.planes = (const uint8_t*)ws + (size_t)n * (size_t)g.coef_bytes;
    a.status = status; a.tile_index = tile_index;
    a.transform = transform; a.grid_cols = grid_cols; a.grid_rows = grid_rows;
    a.level = level; a.pitch = pitch; a.H = H; a.W = W;
    a.pieces_per_row = (width * 3 + 15) / 16 + 1;
    const long long per_tile = (long long)a.pieces_per_row * height;
    for (int t0 = 0; t0 < n; t0 += 65535) {
        const int nt = n - t0 < 65535 ? n - t0 : 65535;
        hipLaunchKernelGGL(store_kernel, dim3((unsigned)((per_tile + 255) / 256), (unsigned)nt), dim3(256), 0, st, a, g, t0);
    }
    return launched();
}
