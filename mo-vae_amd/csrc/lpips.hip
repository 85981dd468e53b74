// The feature distance of the final evaluation's LPIPS (reference utils/metrics.py:290-357 lpips, over the hooks of
// :206-282 VGGFeatureExtractor): per tapped layer, both NHWC feature maps are L2-normalised over the channels of every pixel
// (F.normalize: x / max(||x||, 1e-12)), the squared difference is summed over the channels and averaged over the pixels; the
// layers are averaged, then the images.
//
// One launch per layer and one for all of them at the end, no host read:
//   lpips_layer_k<Q>    a group of GW lanes (the power of two >= min(64, c / 4)) holds one pixel of both maps in registers,
//                       Q float4s per lane and map along C (quad j + 64 k of lane j), so every feature element is read from
//                       HBM exactly once.  The two sums of squares are reduced over the group with shuffles; the difference
//                       is then formed DIRECTLY from the held values, x1 / n1 - x2 / n2, and its squares reduced the same way.
//                       (The expanded form s11 / n1^2 + s22 / n2^2 - 2 s12 / (n1 n2) would cancel for nearly equal maps -- what
//                       a good autoencoder produces -- and would not give an exact 0 for identical ones.)  The arithmetic after
//                       the load is fp64: the kernel stays bound by its loads, a pixel of 512 channels at 1e18 does not
//                       overflow, and the rounding left is that of the fp32 inputs.  A block belongs to ONE image (grid.y) and
//                       writes one fp64 partial: the sum over its pixels, times `scale`.
//   lpips_finalize_k    one block: per image, the partials of each layer in their stored order, times 1 / (h w) of the layer,
//                       the layers in their given order, times 1 / layers; out[1 + i] per image and out[0] their mean.
// No atomics, no memset, no in-launch hand-off: every sum has a fixed order, so two runs give the same bits.
#include "common.h"

#include <math.h>

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_TRIPS = 4;        // pixels a group visits (their loads are issued together) at Q == 1; 4 / Q in general
constexpr int LP_MAX_LAYERS = 8;
constexpr int LP_MAX_C = 1024;     // Q <= 4

struct LayerPlan {
    int gw;     // lanes per pixel
    int q;      // float4s per lane and map: 1, 2 or 4
    int ppb;    // pixels per block
    int ppi;    // blocks (= partials) per image
};

inline LayerPlan plan_of(int h, int w, int c) {
    LayerPlan p;
    const int quads = c / 4;
    p.gw = 1;
    while (p.gw < quads && p.gw < 64) p.gw <<= 1;
    const int per_lane = (quads + p.gw - 1) / p.gw;
    p.q = per_lane <= 1 ? 1 : (per_lane <= 2 ? 2 : 4);
    p.ppb = (LP_THREADS / p.gw) * (LP_TRIPS / p.q);
    p.ppi = (int)(((long long)h * w + p.ppb - 1) / p.ppb);
    return p;
}

__device__ __forceinline__ double group_sum(double v, int gw) {
    for (int o = gw >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int Q>
__global__ __launch_bounds__(LP_THREADS) void lpips_layer_k(const float* __restrict__ f1, const float* __restrict__ f2, int hw, int c,
                                                            int gw, double scale, double* __restrict__ part) {
    constexpr int TR = LP_TRIPS / Q;
    __shared__ double sh[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int sub = t / gw, j = t - sub * gw;  // pixel slot of the block, lane of the group
    const int groups = LP_THREADS / gw, quads = c >> 2;
    const long long img = blockIdx.y;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 a[TR][Q], b[TR][Q];
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        const int px = (blockIdx.x * TR + r) * groups + sub;
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const int qd = j + k * gw;
            a[r][k] = zero, b[r][k] = zero;
            if (px < hw && qd < quads) {  // (a lane past the pixels or the channels holds zeros: they add nothing below)
                const long long o = (img * hw + px) * (long long)c + 4 * qd;
                a[r][k] = *reinterpret_cast<const f32x4*>(f1 + o);
                b[r][k] = *reinterpret_cast<const f32x4*>(f2 + o);
            }
        }
    }
    double total = 0.0;
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int k = 0; k < Q; ++k)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double x = (double)a[r][k][u], y = (double)b[r][k][u];
                s1 = fma(x, x, s1);
                s2 = fma(y, y, s2);
            }
        s1 = group_sum(s1, gw);
        s2 = group_sum(s2, gw);
        // F.normalize's rule: x / max(||x||, eps); an all-zero pixel stays zero
        const double i1 = 1.0 / fmax(sqrt(s1), 1e-12), i2 = 1.0 / fmax(sqrt(s2), 1e-12);
        double d2 = 0.0;
#pragma unroll
        for (int k = 0; k < Q; ++k)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                // both products rounded before the subtraction (no fused multiply-subtract): identical operands give exactly 0
                double d;
                {
#pragma clang fp contract(off)
                    const double x = (double)a[r][k][u] * i1, y = (double)b[r][k][u] * i2;
                    d = x - y;
                }
                d2 = fma(d, d, d2);
            }
        d2 = group_sum(d2, gw);  // every lane of the group now holds the pixel's distance
        total += j == 0 ? d2 : 0.0;
    }
    total = wave_sum(total);
    if (lane == 0) sh[wave] = total;
    __syncthreads();
    if (t == 0) part[img * gridDim.x + blockIdx.x] = scale * ((sh[0] + sh[1]) + (sh[2] + sh[3]));
}

struct FinalArgs {
    const double* part[LP_MAX_LAYERS];
    int ppi[LP_MAX_LAYERS];
    double inv_hw[LP_MAX_LAYERS];
    int layers;
};

// out[0] the mean over the images, out[1 + i] image i
__global__ __launch_bounds__(LP_THREADS) void lpips_finalize_k(FinalArgs a, int n, float* __restrict__ out) {
    __shared__ double sh[4];
    const int t = threadIdx.x;
    double mine = 0.0;
    for (int i = t; i < n; i += LP_THREADS) {
        double v = 0.0;
        for (int l = 0; l < a.layers; ++l) {
            const double* p = a.part[l] + (long long)i * a.ppi[l];
            double s = 0.0;
            for (int q = 0; q < a.ppi[l]; ++q) s += p[q];
            v += s * a.inv_hw[l];
        }
        v /= (double)a.layers;
        out[1 + i] = (float)v;
        mine += v;
    }
    const double all = block_sum_256(mine, sh);
    if (t == 0) out[0] = (float)(all / n);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_shape(const char* who, int n, int h, int w, int c) {
    MOVAE_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0, "%s: empty shape %d x %d x %d x %d", who, n, h, w, c);
    MOVAE_CHECK_ARG(c % 4 == 0 && c <= LP_MAX_C, "%s: the channel count must be a multiple of 4, at most %d (got %d)", who, LP_MAX_C, c);
    MOVAE_CHECK_ARG(n <= 65535, "%s: n %d above the grid limit", who, n);
    MOVAE_CHECK_ARG((long long)h * w <= (1 << 30), "%s: %d x %d pixels per image are too many", who, h, w);
    return MOVAE_OK;
}

}  // namespace

extern "C" size_t movae_lpips_ws_bytes(int n, int h, int w, int c) {
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || c % 4 || c > LP_MAX_C) return 0;
    return (((size_t)n * plan_of(h, w, c).ppi * sizeof(double)) + 255) & ~(size_t)255;
}

extern "C" int movae_lpips_layer(const float* f1, const float* f2, int n, int h, int w, int c, float scale, double* partials,
                                 size_t partials_bytes, movae_stream_t stream) {
    MOVAE_CHECK_ARG(f1 && f2 && partials, "movae_lpips_layer: null pointer");
    if (int rc = check_shape("movae_lpips_layer", n, h, w, c)) return rc;
    MOVAE_CHECK_ARG(aligned16(f1) && aligned16(f2), "movae_lpips_layer: the feature tensors must be 16-byte aligned");
    MOVAE_CHECK_ARG((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "movae_lpips_layer: partials must be 8-byte aligned");
    MOVAE_CHECK_ARG(partials_bytes >= movae_lpips_ws_bytes(n, h, w, c), "movae_lpips_layer: partials hold %zu bytes < %zu", partials_bytes,
                    movae_lpips_ws_bytes(n, h, w, c));
    const LayerPlan p = plan_of(h, w, c);
    const dim3 grid(p.ppi, n), block(LP_THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (p.q) {
        case 1: hipLaunchKernelGGL(lpips_layer_k<1>, grid, block, 0, st, f1, f2, h * w, c, p.gw, (double)scale, partials); break;
        case 2: hipLaunchKernelGGL(lpips_layer_k<2>, grid, block, 0, st, f1, f2, h * w, c, p.gw, (double)scale, partials); break;
        default: hipLaunchKernelGGL(lpips_layer_k<4>, grid, block, 0, st, f1, f2, h * w, c, p.gw, (double)scale, partials); break;
    }
    MOVAE_CHECK_LAUNCH("lpips_layer_k");
    return MOVAE_OK;
}

extern "C" int movae_lpips_finalize(int layers, const double* const* partials, const int* h, const int* w, const int* c, int n, float* out,
                                    movae_stream_t stream) {
    MOVAE_CHECK_ARG(layers >= 1 && layers <= LP_MAX_LAYERS, "movae_lpips_finalize: 1 .. %d layers per call (got %d)", LP_MAX_LAYERS, layers);
    MOVAE_CHECK_ARG(partials && h && w && c && out, "movae_lpips_finalize: null pointer");
    FinalArgs a{};
    a.layers = layers;
    for (int l = 0; l < layers; ++l) {
        MOVAE_CHECK_ARG(partials[l], "movae_lpips_finalize: null partials of layer %d", l);
        if (int rc = check_shape("movae_lpips_finalize", n, h[l], w[l], c[l])) return rc;
        a.part[l] = partials[l];
        a.ppi[l] = plan_of(h[l], w[l], c[l]).ppi;
        a.inv_hw[l] = 1.0 / ((double)h[l] * (double)w[l]);
    }
    hipLaunchKernelGGL(lpips_finalize_k, dim3(1), dim3(LP_THREADS), 0, static_cast<hipStream_t>(stream), a, n, out);
    MOVAE_CHECK_LAUNCH("lpips_finalize_k");
    return MOVAE_OK;
}
