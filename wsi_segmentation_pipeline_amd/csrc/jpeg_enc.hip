// The resident (H, W, 3) or (H, W) u8 level -> baseline JPEG tile scans (include/wsi_hip.h, wsi_jenc_*): the mirror of jpeg.hip.
// Integer arithmetic throughout, libjpeg's default encode path restated (spec: tests/jpeg_enc_oracle.py): the bytes equal libjpeg's.
//   transform_kernel  : one workgroup per segment (16 MCUs) of one MCU row of one tile.  The segment's pixel rows come into LDS in
//                       aligned 16-byte pieces, bytes where a piece is cut by the row segment's ends (rows and columns outside the
//                       level: the nearest level pixel); jccolor's RGB -> YCbCr and jcsample's box downsampling fill u8 planes;
//                       eight lanes per 8x8 block run jfdctint's islow FDCT (rows, then columns through LDS) and jcdctmgr's
//                       quantisation; the int16 coefficients leave in 16-byte stores, MCU by MCU, component by component, zigzag.
//   size_kernel,
//   write_kernel      : one lane per tile runs jpeg_enc_dev.h's encode_tile (the same source the host sanitizer program runs) with a
//                       counting or a storing sink; a workgroup is one wave with `lanes` of its 64 lanes at work, as in jpeg.hip.
//                       The encode form of the four standard Huffman tables sits in LDS.
//   downsample_kernel : f x f box mean of a u8 image, one lane per output byte.
// The workspace of n tiles: n coefficient areas of wsi_jenc_workspace_bytes() each.
#include "internal.h"
#include "jpeg_enc_dev.h"

namespace {
using wsi_jenc::Geometry;

constexpr int SEG_MCUS = 16;                                   // MCUs of one MCU row that a workgroup transforms
constexpr int SEG_PIX = SEG_MCUS * 16;                         // its pixels per row at most (2 x 8 per MCU)
constexpr int ROW_BYTES = SEG_PIX * 3 + 16;                    // a staged row: the pixels' bytes behind the address's phase in 16
constexpr int ROW_PIECES = ROW_BYTES / 16;
constexpr int SEG_BLOCKS = SEG_MCUS * 6;                       // blocks of a segment at most (4:2:0)
constexpr int PASS_BLOCKS = 32;                                // blocks per FDCT pass: 8 lanes each
constexpr int TMP_STRIDE = 72;                                 // ints per block between the passes: 64 + 8, so that eight blocks' columns spread over the banks

struct TransformArgs {
    const uint8_t* level;
    long long pitch;
    int H, W, grid_cols, first_cell, segs;
    uint8_t* ws;
    unsigned short divisor[2][64];                             // 8 q in natural order: luma, chroma
};

// jfdctint.c, jpeg_fdct_islow: CONST_BITS 13, PASS1_BITS 2, the multipliers FIX(x) = round(x * 2^13).  libjpeg's sums fit 32 bits.
#define E_0_298631336 2446
#define E_0_390180644 3196
#define E_0_541196100 4433
#define E_0_765366865 6270
#define E_0_899976223 7373
#define E_1_175875602 9633
#define E_1_501321110 12299
#define E_1_847759065 15137
#define E_1_961570560 16069
#define E_2_053119869 16819
#define E_2_562915447 20995
#define E_3_072711026 25172

// one 1-D pass; FIRST: the row pass (outputs 0 and 4 scaled up by PASS1_BITS, the others descaled by 11), else the column pass
template <bool FIRST>
__device__ inline void fdct_1d(const int (&d)[8], int (&o)[8]) {
    constexpr int SH = FIRST ? 11 : 15, R = 1 << (SH - 1);
    int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (FIRST) {
        o[0] = (tmp10 + tmp11) * 4;
        o[4] = (tmp10 - tmp11) * 4;
    } else {
        o[0] = (tmp10 + tmp11 + 2) >> 2;
        o[4] = (tmp10 - tmp11 + 2) >> 2;
    }
    int z1 = (tmp12 + tmp13) * E_0_541196100;
    o[2] = (z1 + tmp13 * E_0_765366865 + R) >> SH;
    o[6] = (z1 - tmp12 * E_1_847759065 + R) >> SH;
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * E_1_175875602;
    tmp4 *= E_0_298631336; tmp5 *= E_2_053119869; tmp6 *= E_3_072711026; tmp7 *= E_1_501321110;
    z1 *= -E_0_899976223; z2 *= -E_2_562915447; z3 *= -E_1_961570560; z4 *= -E_0_390180644;
    z3 += z5; z4 += z5;
    o[7] = (tmp4 + z1 + z3 + R) >> SH;
    o[5] = (tmp5 + z2 + z4 + R) >> SH;
    o[3] = (tmp6 + z2 + z3 + R) >> SH;
    o[1] = (tmp7 + z1 + z4 + R) >> SH;
}

__global__ __launch_bounds__(256) void transform_kernel(TransformArgs a, Geometry g) {
    __shared__ __attribute__((aligned(16))) uint8_t pix[16 * ROW_BYTES];       // the staged pixel rows
    __shared__ int phase[16];                                                  // a row's first byte in its staged row
    __shared__ uint8_t yp[16 * SEG_PIX];                                       // luma (or grey) samples, SEG_PIX per row
    __shared__ uint8_t cp[2][8 * (SEG_PIX / 2)];                               // Cb, Cr samples after downsampling, SEG_PIX / 2 per row
    __shared__ int tmp[PASS_BLOCKS * TMP_STRIDE];                              // between the FDCT passes
    __shared__ __attribute__((aligned(16))) short out[SEG_BLOCKS * 64];        // the segment's coefficients as they leave
    __shared__ unsigned short divisor[2][64];

    const int tid = threadIdx.x;
    const int seg = (int)(blockIdx.x % (unsigned)a.segs);
    const unsigned rest = blockIdx.x / (unsigned)a.segs;
    const int my = (int)(rest % (unsigned)g.mcuy), tile = (int)(rest / (unsigned)g.mcuy);
    const int rows = 8 * g.vs, mcu_w = 8 * g.hs;
    const int mcu0 = seg * SEG_MCUS;
    const int mcus = g.mcux - mcu0 < SEG_MCUS ? g.mcux - mcu0 : SEG_MCUS;      // >= 1
    const int segw = mcus * mcu_w;                                             // pixels per row of this segment
    const int cell = a.first_cell + tile;
    const long long x0 = (long long)(cell % a.grid_cols) * g.width + (long long)mcu0 * mcu_w;      // the segment's first column in the level
    const long long y0 = (long long)(cell / a.grid_cols) * g.height + (long long)my * rows;
    // the level's columns [lo, hi) serve the segment: its own where they exist, else the level's last
    const long long lo = x0 < a.W - 1 ? x0 : a.W - 1;
    const long long hi = x0 + segw < a.W ? x0 + segw : a.W;                    // > lo
    const int nb = (int)(hi - lo) * g.ncomp;                                   // bytes per row, <= SEG_PIX * 3

    if (tid < 128) divisor[tid >> 6][tid & 63] = a.divisor[tid >> 6][tid & 63];
    for (int idx = tid; idx < rows * ROW_PIECES; idx += 256) {
        const int r = idx / ROW_PIECES, k = idx - r * ROW_PIECES;
        const long long y = y0 + r < a.H - 1 ? y0 + r : a.H - 1;
        const uint8_t* src = a.level + y * a.pitch + lo * g.ncomp;
        const int ph = (int)((uintptr_t)src & 15u);
        if (k == 0) phase[r] = ph;
        const int first = 16 * k, end = ph + nb;                               // the piece [first, first + 16) of the aligned run [0, end)
        if (first >= end) continue;
        const uint8_t* al = src - ph;
        uint8_t* dst = pix + r * ROW_BYTES;
        if (first >= ph && first + 16 <= end) {
            *(u32x4*)(dst + first) = *(const u32x4*)(al + first);
        } else {
            const int b0 = first > ph ? first : ph, b1 = first + 16 < end ? first + 16 : end;
            for (int j = b0; j < b1; ++j) dst[j] = al[j];
        }
    }
    __syncthreads();

    // colour + downsample: one lane per chroma sample takes its hs x vs pixels (one lane per pixel for a grey level)
    {
        const int cw = segw / g.hs;
        const int last = (int)(hi - lo) - 1;                                   // the staged pixel a column past the level reads
        for (int idx = tid; idx < 8 * cw; idx += 256) {
            const int cy = idx / cw, cx = idx - cy * cw;
            int sb = 0, sr = 0;
            for (int dy = 0; dy < g.vs; ++dy) {
                const int r = cy * g.vs + dy;
                const uint8_t* row = pix + r * ROW_BYTES + phase[r];
                for (int dx = 0; dx < g.hs; ++dx) {
                    const int x = cx * g.hs + dx;
                    long long j = x0 + x - lo;                                 // >= 0: lo <= x0
                    j = j < last ? j : last;
                    if (g.ncomp == 1) {
                        yp[r * SEG_PIX + x] = row[j];
                    } else {
                        const int R = row[3 * j], G = row[3 * j + 1], B = row[3 * j + 2];
                        yp[r * SEG_PIX + x] = (uint8_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
                        sb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
                        sr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
                    }
                }
            }
            if (g.ncomp == 3) {
                // jcsample.c: h2v1 bias 0, 1, 0, 1 ..., h2v2 bias 1, 2, 1, 2 ... along the output row (a segment starts at an even column)
                const int shift = g.hs * g.vs == 4 ? 2 : g.hs == 2 ? 1 : 0;
                const int bias = shift == 2 ? 1 + (cx & 1) : shift == 1 ? (cx & 1) : 0;
                cp[0][cy * (SEG_PIX / 2) + cx] = (uint8_t)((sb + bias) >> shift);
                cp[1][cy * (SEG_PIX / 2) + cx] = (uint8_t)((sr + bias) >> shift);
            }
        }
    }
    __syncthreads();

    const int luma_blocks = g.ncomp == 3 ? g.hs * g.vs : 1;
    const int nblk = mcus * g.bpm;
    const int slot = tid >> 3, line = tid & 7;
    for (int b0 = 0; b0 < nblk; b0 += PASS_BLOCKS) {
        const int b = b0 + slot;
        int q = 0;
        if (b < nblk) {                                                        // rows: lane `line` takes row `line` of block b
            const int mcu = b / g.bpm, bi = b - mcu * g.bpm;
            const uint8_t* s;
            if (bi < luma_blocks) {
                const int by = bi / g.hs, bx = bi - by * g.hs;
                s = yp + (by * 8 + line) * SEG_PIX + (mcu * g.hs + bx) * 8;
            } else {
                q = 1;
                s = cp[bi - luma_blocks] + line * (SEG_PIX / 2) + mcu * 8;
            }
            int d[8], o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = (int)s[k] - 128;
            fdct_1d<true>(d, o);
#pragma unroll
            for (int k = 0; k < 8; ++k) tmp[slot * TMP_STRIDE + line * 8 + k] = o[k];
        }
        __syncthreads();
        if (b < nblk) {                                                        // columns: lane `line` takes column `line`, then quantises
            int d[8], o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = tmp[slot * TMP_STRIDE + k * 8 + line];
            fdct_1d<false>(d, o);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int nat = k * 8 + line;
                const int dv = divisor[q][nat];
                const int mag = ((o[k] < 0 ? -o[k] : o[k]) + (dv >> 1)) / dv;
                out[b * 64 + wsi_jenc::natural_zigzag(nat)] = (short)(o[k] < 0 ? -mag : mag);
            }
        }
        __syncthreads();
    }
    // the segment's blocks are one run of the tile's area: MCU (my, mcu0) onwards
    uint8_t* dst = a.ws + (size_t)tile * (size_t)g.tile_bytes + ((size_t)my * g.mcux + mcu0) * (size_t)g.bpm * 128;
    for (int k = tid; k < nblk * 8; k += 256) ((u32x4*)dst)[k] = ((const u32x4*)out)[k];
}

__device__ const wsi_jenc::EncTables g_enc_tables = wsi_jenc::make_enc_tables();

__device__ inline void load_enc_tables(unsigned (*tab)[256]) {
    for (int k = threadIdx.x; k < 4 * 256; k += 64) tab[k >> 8][k & 255] = g_enc_tables.code[k >> 8][k & 255];
    __syncthreads();
}

__global__ __launch_bounds__(64) void size_kernel(const uint8_t* ws, int n, Geometry g, int restart, unsigned* sizes, int lanes) {
    __shared__ unsigned tab[4][256];
    load_enc_tables(tab);
    if ((int)threadIdx.x >= lanes) return;
    const long long i = (long long)blockIdx.x * lanes + threadIdx.x;
    if (i >= n) return;
    sizes[i] = (unsigned)wsi_jenc::encode_tile((const short*)(ws + (size_t)i * (size_t)g.tile_bytes), g, restart, tab, wsi_jenc::CountSink());
}

__global__ __launch_bounds__(64) void write_kernel(const uint8_t* ws, int n, Geometry g, int restart, const unsigned long long* offsets,
                                                   const unsigned* sizes, uint8_t* dst, int lanes) {
    __shared__ unsigned tab[4][256];
    load_enc_tables(tab);
    if ((int)threadIdx.x >= lanes) return;
    const long long i = (long long)blockIdx.x * lanes + threadIdx.x;
    if (i >= n) return;
    wsi_jenc::StoreSink sink;
    sink.p = dst + offsets[i];
    sink.cap = sizes[i];
    wsi_jenc::encode_tile((const short*)(ws + (size_t)i * (size_t)g.tile_bytes), g, restart, tab, sink);
}

__global__ __launch_bounds__(256) void downsample_kernel(const uint8_t* src, long long src_pitch, int channels, int f, uint8_t* dst,
                                                         long long dst_pitch, int dh, int dw) {
    const long long row_bytes = (long long)dw * channels, total = row_bytes * dh;
    const int area = f * f;
    for (long long id = (long long)blockIdx.x * 256 + threadIdx.x; id < total; id += (long long)gridDim.x * 256) {
        const long long y = id / row_bytes, xb = id - y * row_bytes;
        const long long x = xb / channels, c = xb - x * channels;
        const uint8_t* s = src + y * f * src_pitch + x * f * channels + c;
        int sum = 0;
        for (int dy = 0; dy < f; ++dy)
            for (int dx = 0; dx < f; ++dx) sum += s[dy * src_pitch + (long long)dx * channels];
        dst[y * dst_pitch + xb] = (uint8_t)((sum + area / 2) / area);
    }
}

int launched() { return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT; }

// Annex K.1 / K.2, natural order
const unsigned char STD_LUMA_Q[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57,
                                      69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64,
                                      81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const unsigned char STD_CHROMA_Q[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                        99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

bool batch_ok(const void* ws, size_t ws_bytes, int n, int width, int height, int ncomp, int hs, int vs, Geometry* g) {
    if (!ws || n <= 0 || !wsi_jenc::geometry_make(width, height, ncomp, hs, vs, g)) return false;
    return !((uintptr_t)ws & 15u) && ws_bytes / (size_t)g->tile_bytes >= (size_t)n;
}
}  // namespace

int wsi_jenc_quality_tables(int quality, uint8_t* luma_natural, uint8_t* chroma_natural) {
    if (!luma_natural || !chroma_natural) return WSI_EINVAL;
    // jcparam.c jpeg_quality_scaling + jpeg_add_quant_table with force_baseline
    const int q = quality < 1 ? 1 : quality > 100 ? 100 : quality;
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int k = 0; k < 64; ++k) {
        const int l = (STD_LUMA_Q[k] * scale + 50) / 100, c = (STD_CHROMA_Q[k] * scale + 50) / 100;
        luma_natural[k] = (uint8_t)(l < 1 ? 1 : l > 255 ? 255 : l);
        chroma_natural[k] = (uint8_t)(c < 1 ? 1 : c > 255 ? 255 : c);
    }
    return WSI_OK;
}

int wsi_jenc_std_huff(int table, uint8_t* counts16, uint8_t* symbols, int* n_symbols) {
    if (!counts16 || !symbols || !n_symbols || table < 0 || table > 3) return WSI_EINVAL;
    for (int k = 0; k < 16; ++k) counts16[k] = wsi_jenc::STD_HUFF.counts[table][k];
    for (int k = 0; k < wsi_jenc::STD_HUFF.n[table]; ++k) symbols[k] = wsi_jenc::STD_HUFF.symbols[table][k];
    *n_symbols = wsi_jenc::STD_HUFF.n[table];
    return WSI_OK;
}

size_t wsi_jenc_workspace_bytes(int width, int height, int ncomp, int hs, int vs) {
    Geometry g;
    return wsi_jenc::geometry_make(width, height, ncomp, hs, vs, &g) ? (size_t)g.tile_bytes : 0;
}

int wsi_jenc_transform(const uint8_t* level, long long pitch, int H, int W, int grid_cols, int grid_rows, int first_cell, int n, int width,
                       int height, int ncomp, int hs, int vs, const uint8_t* luma_natural, const uint8_t* chroma_natural, void* ws,
                       size_t ws_bytes, void* stream) {
    Geometry g;
    if (!level || !luma_natural || !chroma_natural || !batch_ok(ws, ws_bytes, n, width, height, ncomp, hs, vs, &g)) return WSI_EINVAL;
    if (H <= 0 || W <= 0 || grid_cols <= 0 || grid_rows <= 0 || pitch < (long long)W * ncomp) return WSI_EINVAL;
    if ((long long)(grid_cols - 1) * width >= W || (long long)(grid_rows - 1) * height >= H) return WSI_EINVAL;      // a cell that starts outside the level
    if (first_cell < 0 || (long long)first_cell + n > (long long)grid_cols * grid_rows) return WSI_EINVAL;
    TransformArgs a;
    for (int k = 0; k < 64; ++k) {
        if (luma_natural[k] < 1 || chroma_natural[k] < 1) return WSI_EINVAL;                                         // a uint8_t is never above 255
        a.divisor[0][k] = (unsigned short)(8 * luma_natural[k]);
        a.divisor[1][k] = (unsigned short)(8 * chroma_natural[k]);
    }
    a.level = level; a.pitch = pitch; a.H = H; a.W = W; a.grid_cols = grid_cols; a.first_cell = first_cell;
    a.segs = (g.mcux + SEG_MCUS - 1) / SEG_MCUS;
    a.ws = (uint8_t*)ws;
    const long long groups = (long long)n * g.mcuy * a.segs;
    if (groups > 0x7fffffffLL) return WSI_EINVAL;                                                                    // one launch, one grid dimension
    hipLaunchKernelGGL(transform_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, a, g);
    return launched();
}

int wsi_jenc_entropy_size(const void* ws, size_t ws_bytes, int n, int width, int height, int ncomp, int hs, int vs, int restart,
                          unsigned int* sizes, int lanes, void* stream) {
    Geometry g;
    if (!sizes || !batch_ok(ws, ws_bytes, n, width, height, ncomp, hs, vs, &g) || restart < 0 || restart > 65535 || lanes < 0 || lanes > 64) return WSI_EINVAL;
    lanes = wsi_entropy_lanes(n, lanes);
    hipLaunchKernelGGL(size_kernel, dim3((unsigned)((n + lanes - 1) / lanes)), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)ws, n, g, restart, sizes, lanes);
    return launched();
}

int wsi_jenc_entropy_write(const void* ws, size_t ws_bytes, int n, int width, int height, int ncomp, int hs, int vs, int restart,
                           const unsigned long long* offsets, const unsigned int* sizes, void* ranges_dev, uint8_t* out, size_t out_bytes,
                           int lanes, void* stream) {
    Geometry g;
    if (!offsets || !sizes || !ranges_dev || !out || !batch_ok(ws, ws_bytes, n, width, height, ncomp, hs, vs, &g)) return WSI_EINVAL;
    if (restart < 0 || restart > 65535 || lanes < 0 || lanes > 64 || ((uintptr_t)ranges_dev & 7u)) return WSI_EINVAL;
    for (int i = 0; i < n; ++i)
        if (offsets[i] > out_bytes || sizes[i] > out_bytes - offsets[i]) return WSI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* off_dev = (unsigned long long*)ranges_dev;
    unsigned* size_dev = (unsigned*)(off_dev + n);
    if (hipMemcpyAsync(off_dev, offsets, (size_t)n * 8, hipMemcpyHostToDevice, st) != hipSuccess) return WSI_EFAULT;
    if (hipMemcpyAsync(size_dev, sizes, (size_t)n * 4, hipMemcpyHostToDevice, st) != hipSuccess) return WSI_EFAULT;
    lanes = wsi_entropy_lanes(n, lanes);
    hipLaunchKernelGGL(write_kernel, dim3((unsigned)((n + lanes - 1) / lanes)), dim3(64), 0, st, (const uint8_t*)ws, n, g, restart, off_dev, size_dev, out, lanes);
    return launched();
}

int wsi_jenc_downsample(const uint8_t* src, long long src_pitch, int H, int W, int channels, int factor, uint8_t* dst, long long dst_pitch,
                        void* stream) {
    if (!src || !dst || H <= 0 || W <= 0 || (channels != 1 && channels != 3) || (factor != 2 && factor != 4)) return WSI_EINVAL;
    const int dh = H / factor, dw = W / factor;
    if (dh <= 0 || dw <= 0 || src_pitch < (long long)W * channels || dst_pitch < (long long)dw * channels) return WSI_EINVAL;
    const long long total = (long long)dh * dw * channels;
    const long long want = (total + 255) / 256;
    hipLaunchKernelGGL(downsample_kernel, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(256), 0, (hipStream_t)stream, src, src_pitch, channels,
                       factor, dst, dst_pitch, dh, dw);
    return launched();
}
