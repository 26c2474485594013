// Store-shape probe for the mode-3 conv epilogue: does the memory path care WHICH lane stores which 16-byte piece of an output
// line when the pixels of a tile lie 96 ... 2048 bytes apart?  (store_pattern.hip asked this for contiguous 4 KB tiles only.)
// A wave writes tiles of 32 pixels x one 32-channel line; item t = (pixel tile t / NTL, channel tile t % NTL), grid-strided
// over persistent waves, so neighbouring waves write neighbouring lines of the same pixels, as the conv kernels do.
// 128-byte lines, pixel stride S (256 / 512 / 2048 bytes):
//   a   today: lane (p = l & 31, h = l >> 5) stores {32h, 32h+16, 64+16h, 96+16h} of pixel p: 32 lines x 32 bytes per instruction
//   b   whole lines: instruction j stores piece l & 7 of pixel 8j + (l >> 3): 8 complete lines per instruction
//   c   64-byte sectors: instruction j stores piece l & 3 of sector h of pixel 4 ((l & 31) >> 2) + j (what a quad transpose
//       of the registers gives without LDS): 16 sectors = 8 complete lines per instruction, halves 32 lanes apart
// 96-byte line-planar lines (pixel stride 96 inside a plane per channel tile; a tile is one contiguous 3 KB run):
//   a96 today: {32h, 32h+16} by every lane, {64, 80} by the h = 0 lanes
//   b96 six of eight lanes: instruction j stores piece l & 7 (< 6) of pixel 8j + (l >> 3)
//   c96 64 + 32: quads of the h = 0 lanes store the fp16 sector, lane pairs of the h = 1 lanes the 32 bytes behind it
//   d96 packed: the tile's 192 pieces in address order, three full instructions
// Each with MF = 0 / 8 / 32 mode-3 MFMA steps (2 x f16 32x32x16 + 1 x block-scaled fp6 32x32x64, as conv_dev.h mfma_mx6)
// per tile in front of its stores, at 8 and 12 waves per CU.  Prints GB/s written: median (min - max) of 5 timed launches.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

enum { SH_A, SH_B, SH_C, SH_A96, SH_B96, SH_C96, SH_D96 };

template <int SHAPE, int MF>
__global__ __launch_bounds__(256) void k_store(char* out, long long items, int ntl, long long stride, long long plane, float seed) {
    const int lane = threadIdx.x & 63, p = lane & 31, h = lane >> 5;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long long)gridDim.x * 4;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = seed + (float)(lane + r);
    f16x8 wa, xa;
#pragma unroll
    for (int j = 0; j < 8; ++j) { wa[j] = (_Float16)(seed * (float)j); xa[j] = (_Float16)(float)(lane & 3); }
    const i32x8 wq = {lane, 1, 2, 3, 4, 5, 127, 0}, xq = {p, 5, 4, 3, 2, 1, 127, 0};
    for (long long t = wave0; t < items; t += nw) {
        char* o = out + (t % ntl) * plane + (t / ntl) * 32 * stride;
#pragma unroll 4
        for (int m = 0; m < MF; ++m) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa, xa, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa, wa, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wq, xq, acc, 2, 2, 0, 127, 0, 127);
        }
        u32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = u32x4{__float_as_uint(acc[4 * j]), __float_as_uint(acc[4 * j + 1]), __float_as_uint(acc[4 * j + 2]), __float_as_uint(acc[4 * j + 3])};
        if (SHAPE == SH_A) {
            *(u32x4*)(o + p * stride + 32 * h) = v[0];
            *(u32x4*)(o + p * stride + 32 * h + 16) = v[1];
            *(u32x4*)(o + p * stride + 64 + 16 * h) = v[2];
            *(u32x4*)(o + p * stride + 96 + 16 * h) = v[3];
        } else if (SHAPE == SH_B) {
#pragma unroll
            for (int j = 0; j < 4; ++j) *(u32x4*)(o + (8 * j + (lane >> 3)) * stride + (lane & 7) * 16) = v[j];
        } else if (SHAPE == SH_C) {
#pragma unroll
            for (int j = 0; j < 4; ++j) *(u32x4*)(o + (4 * (p >> 2) + j) * stride + 64 * h + (lane & 3) * 16) = v[j];
        } else if (SHAPE == SH_A96) {
            *(u32x4*)(o + p * 96 + 32 * h) = v[0];
            *(u32x4*)(o + p * 96 + 32 * h + 16) = v[1];
            if (h == 0) {
                *(u32x4*)(o + p * 96 + 64) = v[2];
                *(u32x4*)(o + p * 96 + 80) = v[3];
            }
        } else if (SHAPE == SH_B96) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((lane & 7) < 6) *(u32x4*)(o + (8 * j + (lane >> 3)) * 96 + (lane & 7) * 16) = v[j];
        } else if (SHAPE == SH_C96) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (h == 0 || (lane & 3) < 2) *(u32x4*)(o + (4 * (p >> 2) + j) * 96 + 64 * h + (lane & 3) * 16) = v[j];
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) *(u32x4*)(o + (64 * j + lane) * 16) = v[j];
        }
    }
}

typedef void (*kern_t)(char*, long long, int, long long, long long, float);
template <int SHAPE>
static kern_t pick(int mf) { return mf == 0 ? k_store<SHAPE, 0> : mf == 8 ? k_store<SHAPE, 8> : k_store<SHAPE, 32>; }

int main(int argc, char** argv) {
    const long long n = argc > 1 ? atoll(argv[1]) : 2000;                  // images, as the trunk's batch
    struct Fmt { const char* name; long long pixels_per_img, stride; int ntl; bool f96; };
    const Fmt fmts[] = {{"layer-1  96 B line-planar", 4096, 96, 2, true},
                        {"layer-1 256 B", 4096, 256, 2, false},
                        {"layer-2 512 B", 1024, 512, 4, false},
                        {"layer-4 2048 B", 64, 2048, 16, false}};
    size_t cap = 0;
    for (const Fmt& f : fmts) cap = std::max(cap, (size_t)(n * f.pixels_per_img * f.stride * (f.f96 ? 2 : 1)));
    char* out;
    if (hipMalloc(&out, cap) != hipSuccess) { fprintf(stderr, "hipMalloc of %zu bytes failed\n", cap); return 1; }
    hipMemset(out, 0, cap);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    int cus = 256;
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
    printf("tools/probes/store_shape %lld  (%d CUs; GB/s written: median (min - max) of 5 timed launches after one warm-up)\n", n, cus);
    for (const Fmt& f : fmts) {
        const long long pixels = n * f.pixels_per_img, tiles = pixels / 32, items = tiles * f.ntl;
        const long long plane = f.f96 ? pixels * 96 : 128;
        const double bytes = (double)items * 32 * (f.f96 ? 96 : 128);
        printf("%s: %lld items, %.0f MB written\n", f.name, items, bytes * 1e-6);
        struct Sh { const char* name; int id; };
        const Sh s128[] = {{"a   today, 4 x 16 B per lane", SH_A}, {"b   whole lines, 8 lanes", SH_B}, {"c   64 B sectors, lane quads", SH_C}};
        const Sh s96[] = {{"a96 today", SH_A96}, {"b96 six of eight lanes", SH_B96}, {"c96 64 + 32", SH_C96}, {"d96 packed run", SH_D96}};
        for (int mf : {0, 8, 32})
            for (int wpc : {8, 12})
                for (int si = 0; si < (f.f96 ? 4 : 3); ++si) {
                    const Sh& s = f.f96 ? s96[si] : s128[si];
                    kern_t k = s.id == SH_A ? pick<SH_A>(mf) : s.id == SH_B ? pick<SH_B>(mf) : s.id == SH_C ? pick<SH_C>(mf)
                             : s.id == SH_A96 ? pick<SH_A96>(mf) : s.id == SH_B96 ? pick<SH_B96>(mf) : s.id == SH_C96 ? pick<SH_C96>(mf) : pick<SH_D96>(mf);
                    float ms[6];
                    for (int it = 0; it < 6; ++it) {
                        hipEventRecord(e0);
                        hipLaunchKernelGGL(k, dim3(cus * wpc / 4), dim3(256), 0, 0, out, items, f.ntl, f.stride, plane, 0.f);
                        hipEventRecord(e1);
                        if (hipEventSynchronize(e1) != hipSuccess) { fprintf(stderr, "launch failed\n"); return 1; }
                        hipEventElapsedTime(&ms[it], e0, e1);
                    }
                    std::sort(ms + 1, ms + 6);
                    printf("  mfma %2d  %2d waves/CU  %-30s %7.3f ms  %7.1f GB/s (%7.1f - %7.1f)\n", mf, wpc, s.name, ms[3],
                           bytes / ms[3] * 1e-6, bytes / ms[5] * 1e-6, bytes / ms[1] * 1e-6);
                }
    }
    return 0;
}
