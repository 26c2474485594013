// Stain normalisation of u8 RGB pixels resident in device memory: Macenko (Macenko et al., ISBI 2009) and Reinhard (Reinhard et al.,
// IEEE CG&A 2001, in Ruderman's l-alpha-beta space).  The reference has no counterpart; the specification is tests/stain_oracle.py.
//   od_moments / lab_moments : count, sum x and sum x (x) x over the tissue pixels of every image, x = optical density (table values)
//                              or l-alpha-beta (float64), float64 sums in a fixed order: the same input gives the same bits
//   angle_hist / conc_hist   : integer histograms of the stain-plane angle and of the two stain concentrations
//   macenko_apply / reinhard_apply : u8 in, u8 out, dst == src allowed
//
// One walk serves all six.  Image i is npix packed pixels at byte i * npix * 3, so its start is 16-byte aligned for no one.  The first
// `head` pixels (0 to 15: the h with (address + 3 h) % 16 == 0) and a ragged end go through byte accesses; between them the image is
// pieces of 16 pixels = 48 bytes = three 16-byte accesses per lane.  A workgroup owns a chunk of CHUNK_PIECES consecutive pieces
// (32768 pixels), piece (step, thread) = step * 256 + thread, so a wave instruction covers 64 x 16 contiguous bytes of each of three
// streams 16 bytes apart.  The head belongs to thread 0 of chunk 0.  A lane reads its whole piece before it writes it and pieces
// are disjoint: an apply may run in place.
#include "internal.h"
#include "../../include/wsi_hip.h"

namespace {
constexpr int PIECE = 16;                                      // pixels per piece
constexpr int STEPS = 8;                                       // pieces per thread and chunk
constexpr int CHUNK_PIECES = 256 * STEPS;
constexpr long long MAX_NPIX = 1LL << 40;
constexpr int NMOM = 10;                                       // n, sum x (3), sum x (x) x (00 01 02 11 12 22)

__device__ inline int head_pixels(const uint8_t* base, long long npix) {
    const int h = (int)(((16u - (unsigned)((uintptr_t)base & 15u)) & 15u) * 11u & 15u);      // 3 h = -address (mod 16), 3 * 11 = 1 (mod 16)
    return (long long)h < npix ? h : (int)npix;
}

// a piece's 48 bytes as 12 dwords; bytes past `count` pixels read as 255 (no tissue)
__device__ inline void load_piece(const uint8_t* p, int count, bool vec, unsigned (&w)[12]) {
    if (vec && count == PIECE) {
        const u32x4* q = (const u32x4*)p;
        const u32x4 a = q[0], b = q[1], c = q[2];
#pragma unroll
        for (int e = 0; e < 4; ++e) { w[e] = a[e]; w[4 + e] = b[e]; w[8 + e] = c[e]; }
    } else {
#pragma unroll
        for (int e = 0; e < 12; ++e) w[e] = 0;
#pragma unroll
        for (int j = 0; j < 3 * PIECE; ++j) {
            const unsigned v = j < 3 * count ? p[j] : 255u;
            w[j >> 2] |= v << (8 * (j & 3));
        }
    }
}
__device__ inline void store_piece(uint8_t* p, int count, bool vec, const unsigned (&w)[12]) {
    if (vec && count == PIECE) {
        u32x4* q = (u32x4*)p;
        q[0] = u32x4{w[0], w[1], w[2], w[3]};
        q[1] = u32x4{w[4], w[5], w[6], w[7]};
        q[2] = u32x4{w[8], w[9], w[10], w[11]};
    } else {
#pragma unroll
        for (int j = 0; j < 3 * PIECE; ++j)
            if (j < 3 * count) p[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
}
__device__ inline unsigned byte_of(const unsigned (&w)[12], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 255u; }

// f(first pixel, pixels) for every piece of this workgroup's chunk of image blockIdx.y
template <class F>
__device__ inline void for_pieces(const uint8_t* base, long long npix, F&& f) {
    const int head = head_pixels(base, npix);
    if (blockIdx.x == 0 && threadIdx.x == 0 && head > 0) f(0, head);
#pragma unroll 1
    for (int s = 0; s < STEPS; ++s) {
        const long long piece = (long long)blockIdx.x * CHUNK_PIECES + s * 256 + threadIdx.x;
        const long long p0 = head + piece * PIECE;
        if (p0 >= npix) break;
        f(p0, (int)(npix - p0 < PIECE ? npix - p0 : PIECE));
    }
}
static long long chunks_of(long long npix) {                    // the head shortens the body, never lengthens it
    const long long pieces = (npix + PIECE - 1) / PIECE;
    return pieces <= CHUNK_PIECES ? 1 : (pieces + CHUNK_PIECES - 1) / CHUNK_PIECES;
}

// the sum of one double per thread, in a fixed order: lanes by halving strides, then the four waves in order; every thread gets it
__device__ inline double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ------------------------------------------------------------------------------------------------------------------------ moments
// Reinhard's forward transform in float64: rgb = (v + 1) / 256 -> LMS (the paper's matrix) -> log10 -> l-alpha-beta
__device__ inline void lab_f64(unsigned r, unsigned g, unsigned b, double (&x)[3]) {
    const double R = (r + 1) * (1.0 / 256), G = (g + 1) * (1.0 / 256), B = (b + 1) * (1.0 / 256);
    const double L = log10(0.3811 * R + 0.5783 * G + 0.0402 * B);
    const double M = log10(0.1967 * R + 0.7244 * G + 0.0782 * B);
    const double S = log10(0.0241 * R + 0.1288 * G + 0.8444 * B);
    x[0] = (L + M + S) * 0.57735026918962576451;               // 1 / sqrt(3)
    x[1] = (L + M - 2.0 * S) * 0.40824829046386301637;         // 1 / sqrt(6)
    x[2] = (L - M) * 0.70710678118654752440;                   // 1 / sqrt(2)
}

template <bool LAB>
__global__ __launch_bounds__(256) void moments_kernel(const uint8_t* img, long long npix, int v_max, const float* od_lut, double* partials) {
    __shared__ float od[256];
    __shared__ double red[4];
    if (!LAB) od[threadIdx.x] = od_lut[threadIdx.x];
    __syncthreads();
    const uint8_t* base = img + (size_t)blockIdx.y * (size_t)npix * 3;
    double acc[NMOM];
#pragma unroll
    for (int k = 0; k < NMOM; ++k) acc[k] = 0.0;
    for_pieces(base, npix, [&](long long p0, int count) {
        unsigned w[12];
        load_piece(base + p0 * 3, count, true, w);
#pragma unroll
        for (int k = 0; k < PIECE; ++k) {
            const unsigned r = byte_of(w, 3 * k), g = byte_of(w, 3 * k + 1), b = byte_of(w, 3 * k + 2);
            if ((int)max(r, max(g, b)) > v_max) continue;
            double x[3];
            if (LAB) lab_f64(r, g, b, x);
            else { x[0] = od[r]; x[1] = od[g]; x[2] = od[b]; }
            acc[0] += 1.0;
            acc[1] += x[0]; acc[2] += x[1]; acc[3] += x[2];
            acc[4] += x[0] * x[0]; acc[5] += x[0] * x[1]; acc[6] += x[0] * x[2];
            acc[7] += x[1] * x[1]; acc[8] += x[1] * x[2]; acc[9] += x[2] * x[2];
        }
    });
    double* out = partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NMOM;
#pragma unroll
    for (int k = 0; k < NMOM; ++k) {
        const double s = block_sum(acc[k], red);
        if (threadIdx.x == 0) out[k] = s;
    }
}

// one workgroup per image adds the chunk partials: thread t takes chunks t, t + 256, ... in order
__global__ __launch_bounds__(256) void moments_merge_kernel(const double* partials, long long chunks, double* moments) {
    __shared__ double red[4];
    const double* in = partials + (size_t)blockIdx.x * chunks * NMOM;
    double acc[NMOM];
#pragma unroll
    for (int k = 0; k < NMOM; ++k) acc[k] = 0.0;
    for (long long c = threadIdx.x; c < chunks; c += 256)
#pragma unroll
        for (int k = 0; k < NMOM; ++k) acc[k] += in[c * NMOM + k];
#pragma unroll
    for (int k = 0; k < NMOM; ++k) {
        const double s = block_sum(acc[k], red);
        if (threadIdx.x == 0) moments[(size_t)blockIdx.x * NMOM + k] = s;
    }
}

// --------------------------------------------------------------------------------------------------------------------- histograms
// CONC = false: bin of phi = atan2(od . V2, od . V1) over [-pi, pi); prm = V as [3][2] per image
// CONC = true : bins of C = P . od over [0, conc_max), both rows, values outside clamped into the end bins; prm = P as [2][3] per image
template <bool CONC>
__global__ __launch_bounds__(256) void hist_kernel(const uint8_t* img, long long npix, int v_max, const float* od_lut, const float* prm,
                                                   int bins, float conc_max, unsigned long long* hist) {
    extern __shared__ unsigned lh[];                            // bins (angle) or 2 * bins (concentration) counters
    __shared__ float od[256];
    const int nb = CONC ? 2 * bins : bins;
    od[threadIdx.x] = od_lut[threadIdx.x];
    for (int k = threadIdx.x; k < nb; k += 256) lh[k] = 0;
    __syncthreads();
    const uint8_t* base = img + (size_t)blockIdx.y * (size_t)npix * 3;
    float q[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) q[k] = prm[blockIdx.y * 6 + k];
    const float scale = CONC ? (float)bins / conc_max : (float)bins * 0.15915494309189533577f;
    for_pieces(base, npix, [&](long long p0, int count) {
        unsigned w[12];
        load_piece(base + p0 * 3, count, true, w);
#pragma unroll
        for (int k = 0; k < PIECE; ++k) {
            const unsigned r = byte_of(w, 3 * k), g = byte_of(w, 3 * k + 1), b = byte_of(w, 3 * k + 2);
            if ((int)max(r, max(g, b)) > v_max) continue;
            const float x0 = od[r], x1 = od[g], x2 = od[b];
            if (CONC) {
                const float c0 = __builtin_fmaf(q[2], x2, __builtin_fmaf(q[1], x1, q[0] * x0));
                const float c1 = __builtin_fmaf(q[5], x2, __builtin_fmaf(q[4], x1, q[3] * x0));
                atomicAdd(&lh[min(max((int)floorf(c0 * scale), 0), bins - 1)], 1u);
                atomicAdd(&lh[bins + min(max((int)floorf(c1 * scale), 0), bins - 1)], 1u);
            } else {
                const float a = __builtin_fmaf(q[4], x2, __builtin_fmaf(q[2], x1, q[0] * x0));      // od . V1
                const float c = __builtin_fmaf(q[5], x2, __builtin_fmaf(q[3], x1, q[1] * x0));      // od . V2
                const float phi = atan2f(c, a);
                atomicAdd(&lh[min(max((int)floorf((phi + 3.14159265358979323846f) * scale), 0), bins - 1)], 1u);
            }
        }
    });
    __syncthreads();
    unsigned long long* out = hist + (size_t)blockIdx.y * nb;
    for (int k = threadIdx.x; k < nb; k += 256)
        if (lh[k]) atomicAdd(&out[k], (unsigned long long)lh[k]);
}

// ------------------------------------------------------------------------------------------------------------------------ applies
__device__ inline unsigned to_u8(float v) { return (unsigned)fminf(fmaxf(floorf(v), 0.f), 255.f); }

// MACENKO: prm = m [3][3] per image, out_c = floor(io * 2^(m_c . od) + 0.5)
// else   : prm = G [3][3], g [3] per image, log2 LMS' = G . log2 LMS + g, out = floor(256 * (LMS -> RGB) LMS' - 1 + 0.5)
// a pixel with max(r, g, b) > v_max[image] is copied through
template <bool MACENKO>
__global__ __launch_bounds__(256) void apply_kernel(const uint8_t* src, uint8_t* dst, long long npix, const int* v_max, const float* od_lut,
                                                    const float* prm, float io, int vec) {
    __shared__ float od[256];
    if (MACENKO) od[threadIdx.x] = od_lut[threadIdx.x];
    __syncthreads();
    const size_t off = (size_t)blockIdx.y * (size_t)npix * 3;
    const uint8_t* base = src + off;
    const int vm = v_max[blockIdx.y];
    constexpr int NP = MACENKO ? 9 : 12;
    float q[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) q[k] = prm[blockIdx.y * NP + k];
    for_pieces(base, npix, [&](long long p0, int count) {
        unsigned w[12], o[12];
        load_piece(base + p0 * 3, count, vec, w);
#pragma unroll
        for (int e = 0; e < 12; ++e) o[e] = 0;
#pragma unroll
        for (int k = 0; k < PIECE; ++k) {
            unsigned c[3] = {byte_of(w, 3 * k), byte_of(w, 3 * k + 1), byte_of(w, 3 * k + 2)};
            if ((int)max(c[0], max(c[1], c[2])) <= vm) {
                if (MACENKO) {
                    const float x0 = od[c[0]], x1 = od[c[1]], x2 = od[c[2]];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float s = __builtin_fmaf(q[3 * ch + 2], x2, __builtin_fmaf(q[3 * ch + 1], x1, q[3 * ch] * x0));
                        c[ch] = to_u8(__builtin_fmaf(io, __builtin_amdgcn_exp2f(s), 0.5f));
                    }
                } else {
                    const float R = (float)(c[0] + 1) * 0.00390625f, G = (float)(c[1] + 1) * 0.00390625f, B = (float)(c[2] + 1) * 0.00390625f;
                    const float l = __builtin_amdgcn_logf(__builtin_fmaf(0.0402f, B, __builtin_fmaf(0.5783f, G, 0.3811f * R)));
                    const float m = __builtin_amdgcn_logf(__builtin_fmaf(0.0782f, B, __builtin_fmaf(0.7244f, G, 0.1967f * R)));
                    const float s = __builtin_amdgcn_logf(__builtin_fmaf(0.8444f, B, __builtin_fmaf(0.1288f, G, 0.0241f * R)));
                    float t[3];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch)
                        t[ch] = __builtin_amdgcn_exp2f(__builtin_fmaf(q[3 * ch + 2], s, __builtin_fmaf(q[3 * ch + 1], m, __builtin_fmaf(q[3 * ch], l, q[9 + ch]))));
                    // 256 * (LMS -> RGB, the paper's matrix) and the - 1 + 0.5
                    c[0] = to_u8(__builtin_fmaf(256.f * 0.1193f, t[2], __builtin_fmaf(256.f * -3.5873f, t[1], __builtin_fmaf(256.f * 4.4679f, t[0], -0.5f))));
                    c[1] = to_u8(__builtin_fmaf(256.f * -0.1624f, t[2], __builtin_fmaf(256.f * 2.3809f, t[1], __builtin_fmaf(256.f * -1.2186f, t[0], -0.5f))));
                    c[2] = to_u8(__builtin_fmaf(256.f * 1.2045f, t[2], __builtin_fmaf(256.f * -0.2439f, t[1], __builtin_fmaf(256.f * 0.0497f, t[0], -0.5f))));
                }
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[(3 * k + ch) >> 2] |= c[ch] << (8 * ((3 * k + ch) & 3));
        }
        store_piece(dst + off + p0 * 3, count, vec, o);
    });
}

static bool shape_ok(long long npix, int n_images) {
    return npix > 0 && npix <= MAX_NPIX && n_images > 0 && n_images <= 65535 && chunks_of(npix) <= 0x7fffffffLL;
}
static int launched() { return hipGetLastError() == hipSuccess ? WSI_OK : WSI_EFAULT; }

template <bool LAB>
static int moments_run(const uint8_t* img, long long npix, int n_images, int v_max, const float* od_lut, double* moments_out, void* scratch,
                       hipStream_t st) {
    if (!img || !moments_out || !scratch || (!LAB && !od_lut) || !shape_ok(npix, n_images) || v_max < 0 || v_max > 255) return WSI_EINVAL;
    const long long chunks = chunks_of(npix);
    hipLaunchKernelGGL(moments_kernel<LAB>, dim3((unsigned)chunks, n_images), dim3(256), 0, st, img, npix, v_max, od_lut, (double*)scratch);
    hipLaunchKernelGGL(moments_merge_kernel, dim3(n_images), dim3(256), 0, st, (const double*)scratch, chunks, moments_out);
    return launched();
}

template <bool CONC>
static int hist_run(const uint8_t* img, long long npix, int n_images, int v_max, const float* od_lut, const float* prm, int bins,
                    float conc_max, unsigned long long* hist_out, hipStream_t st) {
    if (!img || !od_lut || !prm || !hist_out || !shape_ok(npix, n_images) || v_max < 0 || v_max > 255) return WSI_EINVAL;
    if (bins < 1 || bins > 4096 || (CONC && !(conc_max > 0.f))) return WSI_EINVAL;
    const size_t nb = (size_t)(CONC ? 2 : 1) * bins;
    if (hipMemsetAsync(hist_out, 0, nb * n_images * sizeof(unsigned long long), st) != hipSuccess) return WSI_EFAULT;
    hipLaunchKernelGGL(hist_kernel<CONC>, dim3((unsigned)chunks_of(npix), n_images), dim3(256), nb * sizeof(unsigned), st, img, npix, v_max,
                       od_lut, prm, bins, conc_max, hist_out);
    return launched();
}

template <bool MACENKO>
static int apply_run(const uint8_t* src, uint8_t* dst, long long npix, int n_images, const int* v_max, const float* od_lut, const float* prm,
                     float io, hipStream_t st) {
    if (!src || !dst || !v_max || !prm || (MACENKO && (!od_lut || !(io > 0.f))) || !shape_ok(npix, n_images)) return WSI_EINVAL;
    const unsigned long long bytes = 3ull * (unsigned long long)npix * n_images;
    const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
    if (s != d && s < d + bytes && d < s + bytes) return WSI_EINVAL;           // a partial overlap
    const int vec = ((s ^ d) & 15) == 0;                       // the 16-byte pieces of src are those of dst; otherwise bytes throughout
    hipLaunchKernelGGL(apply_kernel<MACENKO>, dim3((unsigned)chunks_of(npix), n_images), dim3(256), 0, st, src, dst, npix, v_max, od_lut, prm,
                       io, vec);
    return launched();
}
}  // namespace

size_t wsi_stain_moments_scratch_bytes(long long npix, int n_images) {
    return shape_ok(npix, n_images) ? (size_t)chunks_of(npix) * n_images * NMOM * sizeof(double) : 0;
}
int wsi_stain_od_moments(const uint8_t* img, long long npix, int n_images, int v_max, const float* od_lut, double* moments_out, void* scratch,
                         void* stream) {
    return moments_run<false>(img, npix, n_images, v_max, od_lut, moments_out, scratch, (hipStream_t)stream);
}
int wsi_stain_lab_moments(const uint8_t* img, long long npix, int n_images, int v_max, double* moments_out, void* scratch, void* stream) {
    return moments_run<true>(img, npix, n_images, v_max, nullptr, moments_out, scratch, (hipStream_t)stream);
}
int wsi_stain_angle_hist(const uint8_t* img, long long npix, int n_images, int v_max, const float* od_lut, const float* plane_3x2, int bins,
                         unsigned long long* hist_out, void* stream) {
    return hist_run<false>(img, npix, n_images, v_max, od_lut, plane_3x2, bins, 0.f, hist_out, (hipStream_t)stream);
}
int wsi_stain_conc_hist(const uint8_t* img, long long npix, int n_images, int v_max, const float* od_lut, const float* pinv_2x3, int bins,
                        float conc_max, unsigned long long* hist_out, void* stream) {
    return hist_run<true>(img, npix, n_images, v_max, od_lut, pinv_2x3, bins, conc_max, hist_out, (hipStream_t)stream);
}
int wsi_stain_macenko_apply(const uint8_t* src, uint8_t* dst, long long npix, int n_images, const int* v_max, const float* od_lut,
                            const float* m_3x3, float io, void* stream) {
    return apply_run<true>(src, dst, npix, n_images, v_max, od_lut, m_3x3, io, (hipStream_t)stream);
}
int wsi_stain_reinhard_apply(const uint8_t* src, uint8_t* dst, long long npix, int n_images, const int* v_max, const float* g_3x3_3, void* stream) {
    return apply_run<false>(src, dst, npix, n_images, v_max, nullptr, g_3x3_3, 1.f, (hipStream_t)stream);
}
