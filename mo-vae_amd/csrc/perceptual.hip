// The perceptual (VGG16 feature) loss around its convolutions (perceptual.py; the reference's utils/objectives.py:53-79 PerceptualLoss):
//
//   vgg_prep     _norm_input without a host sync: x -> (x + 1) / 2 if the WHOLE tensor's minimum is negative, clamp to [0, 1], then
//                (x - mean_c) / std_c with the ImageNet statistics (C = 3, NHWC: channel = element index % 3).  Two launches for a group
//                of up to 8 same-shape tensors: prep_flag_k writes one "has a negative" int per block into the workspace; prep_fwd_k
//                ORs its tensor's partials (at most 256 ints, L2-resident), normalises, and its first block of each tensor writes the
//                tensor's flag out for the backward.  No atomics, no memset.  Bytes per tensor of n elements: 4n read by the flag
//                pass, 4n read + 4n written by the normalise pass = 12n; the backward 8n read (dy, x) + 4n written = 12n.
//   maxpool2x2   2x2 / stride 2 / floor-mode max-pool on NHWC with C % 4 == 0: one thread per (image, output pixel, channel quad),
//                16-byte accesses along C.  The backward runs over the CEIL grid, so the row / column an odd size drops is written
//                (with zeros) by the thread that would have owned it: every element of dx is stored exactly once, no memset, no
//                atomics.  The first element in the scan order (0,0), (0,1), (1,0), (1,1) that equals the window's maximum takes dy
//                (torch's tie rule).  Bytes with P = n * (h/2) * (w/2) * c pooled elements: forward 16P read + 4P written; backward
//                4P (dy) + 4P (y) + 16P (x) read + 4 n h w c written.
#include "common.h"

namespace {

constexpr int PREP_MAX_G = 8;
constexpr int PREP_MAX_NB = 256;  // blocks per tensor of both prep passes (the fold reads one int per thread)

struct PrepArgs {
    const float* x[PREP_MAX_G];
    float* y[PREP_MAX_G];
    int* flags;  // [G], written by the forward
    int* part;   // [G][nb]
    long n;
    int vec;     // every base 16-byte aligned: quads as one access
};

struct PrepBwdArgs {
    const float* dy[PREP_MAX_G];
    const float* x[PREP_MAX_G];
    float* dx[PREP_MAX_G];
    int slot[PREP_MAX_G];  // index of the tensor's flag
    const int* flags;
    long n;
    int vec;
};

__device__ __forceinline__ float prep_mean(int c) { return c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f); }
__device__ __forceinline__ float prep_std(int c) { return c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f); }

__device__ __forceinline__ float prep_one(float v, int c, int rescale) {
    if (rescale) v = (v + 1.f) * 0.5f;
    v = fminf(fmaxf(v, 0.f), 1.f);
    return (v - prep_mean(c)) / prep_std(c);
}

__device__ __forceinline__ float prep_grad_one(float g, float v, int c, int rescale) {
    if (rescale) v = (v + 1.f) * 0.5f;
    const float s = rescale ? 0.5f : 1.f;
    return (v >= 0.f && v <= 1.f) ? g * s / prep_std(c) : 0.f;
}

__global__ __launch_bounds__(256) void prep_flag_k(PrepArgs a) {
    const int g = blockIdx.y;
    const float* __restrict__ x = a.x[g];
    const long n = a.n, stride = (long)gridDim.x * 256;
    int neg = 0;
    if (a.vec) {
        const long nq = n >> 2;
        for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += stride) {
            const float4 v = *reinterpret_cast<const float4*>(x + 4 * q);
            neg |= (v.x < 0.f) | (v.y < 0.f) | (v.z < 0.f) | (v.w < 0.f);
        }
        for (long i = (nq << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) neg |= x[i] < 0.f;
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) neg |= x[i] < 0.f;
    }
    neg = __syncthreads_or(neg);
    if (threadIdx.x == 0) a.part[g * gridDim.x + blockIdx.x] = neg ? 1 : 0;
}

__global__ __launch_bounds__(256) void prep_fwd_k(PrepArgs a) {
    const int g = blockIdx.y, nb = gridDim.x;  // (the flag pass ran on the same grid)
    const int rescale = __syncthreads_or((int)threadIdx.x < nb ? a.part[g * nb + threadIdx.x] : 0) ? 1 : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.flags[g] = rescale;
    const float* __restrict__ x = a.x[g];
    float* __restrict__ y = a.y[g];
    const long n = a.n, stride = (long)nb * 256;
    if (a.vec) {
        const long nq = n >> 2;
        for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += stride) {
            const float4 v = *reinterpret_cast<const float4*>(x + 4 * q);
            const int c0 = (int)(q % 3);  // (4 q) % 3
            const int c1 = c0 == 2 ? 0 : c0 + 1, c2 = c1 == 2 ? 0 : c1 + 1;
            *reinterpret_cast<float4*>(y + 4 * q) =
                make_float4(prep_one(v.x, c0, rescale), prep_one(v.y, c1, rescale), prep_one(v.z, c2, rescale), prep_one(v.w, c0, rescale));
        }
        for (long i = (nq << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) y[i] = prep_one(x[i], (int)(i % 3), rescale);
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) y[i] = prep_one(x[i], (int)(i % 3), rescale);
    }
}

__global__ __launch_bounds__(256) void prep_bwd_k(PrepBwdArgs a) {
    const int g = blockIdx.y;
    const int rescale = a.flags[a.slot[g]];
    const float* __restrict__ dy = a.dy[g];
    const float* __restrict__ x = a.x[g];
    float* __restrict__ dx = a.dx[g];
    const long n = a.n, stride = (long)gridDim.x * 256;
    if (a.vec) {
        const long nq = n >> 2;
        for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += stride) {
            const float4 v = *reinterpret_cast<const float4*>(x + 4 * q);
            const float4 d = *reinterpret_cast<const float4*>(dy + 4 * q);
            const int c0 = (int)(q % 3);
            const int c1 = c0 == 2 ? 0 : c0 + 1, c2 = c1 == 2 ? 0 : c1 + 1;
            *reinterpret_cast<float4*>(dx + 4 * q) = make_float4(prep_grad_one(d.x, v.x, c0, rescale), prep_grad_one(d.y, v.y, c1, rescale),
                                                                 prep_grad_one(d.z, v.z, c2, rescale), prep_grad_one(d.w, v.w, c0, rescale));
        }
        for (long i = (nq << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
            dx[i] = prep_grad_one(dy[i], x[i], (int)(i % 3), rescale);
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dx[i] = prep_grad_one(dy[i], x[i], (int)(i % 3), rescale);
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// blocks per tensor: a quad per thread and four trips, at most PREP_MAX_NB
inline int prep_blocks(size_t n) {
    size_t b = (n + 4095) / 4096;
    return (int)(b > (size_t)PREP_MAX_NB ? PREP_MAX_NB : (b < 1 ? 1 : b));
}

// ---- max-pool ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float max4(float a, float b, float c, float d) {
    float m = a;
    if (b > m) m = b;
    if (c > m) m = c;
    if (d > m) m = d;
    return m;
}

// thread = (image, ho, wo, channel quad) of the pooled tensor, quads fastest
__global__ __launch_bounds__(256) void maxpool_fwd_k(const float* __restrict__ x, float* __restrict__ y, long total, int h, int w, int c,
                                                     int ho, int wo) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int cq = c >> 2;
    const int q = (int)(t % cq);
    long r = t / cq;
    const int ow = (int)(r % wo);
    r /= wo;
    const int oh = (int)(r % ho);
    const long img = r / ho;
    const float* p = x + ((img * h + 2 * oh) * w + 2 * ow) * (long)c + 4 * q;
    const float4 a = ld4(p), b = ld4(p + c), d = ld4(p + (long)w * c), e = ld4(p + (long)w * c + c);
    st4(y + t * 4, make_float4(max4(a.x, b.x, d.x, e.x), max4(a.y, b.y, d.y, e.y), max4(a.z, b.z, d.z, e.z), max4(a.w, b.w, d.w, e.w)));
}

// one lane of a window: dy to the first of (a, b, d, e) that equals the maximum m
__device__ __forceinline__ void route(float g, float m, float a, float b, float d, float e, float& ga, float& gb, float& gd, float& ge) {
    const bool ta = a == m, tb = !ta && b == m, td = !ta && !tb && d == m, te = !ta && !tb && !td && e == m;
    ga = ta ? g : 0.f, gb = tb ? g : 0.f, gd = td ? g : 0.f, ge = te ? g : 0.f;
}

// thread = (image, hc, wc, channel quad) over the CEIL grid hc = (h + 1) / 2, wc = (w + 1) / 2: it stores the up to four pixels
// (2 hc + {0, 1}, 2 wc + {0, 1}) of dx that exist; a window the floor-mode pool dropped (odd h: its last row, odd w: its last column)
// gets zeros
__global__ __launch_bounds__(256) void maxpool_bwd_k(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y,
                                                     float* __restrict__ dx, long total, int h, int w, int c, int ho, int wo, int hc, int wc) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int cq = c >> 2;
    const int q = (int)(t % cq);
    long r = t / cq;
    const int ow = (int)(r % wc);
    r /= wc;
    const int oh = (int)(r % hc);
    const long img = r / hc;
    const long base = ((img * h + 2 * oh) * w + 2 * ow) * (long)c + 4 * q;
    const long down = (long)w * c;
    const bool has_r = 2 * ow + 1 < w, has_d = 2 * oh + 1 < h;  // the right column / the lower row of this 2x2 patch exists
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    if (oh < ho && ow < wo) {  // a pooled window: all four pixels exist
        const long o = ((img * ho + oh) * wo + ow) * (long)c + 4 * q;
        const float4 g = ld4(dy + o), m = ld4(y + o);
        const float4 a = ld4(x + base), b = ld4(x + base + c), d = ld4(x + base + down), e = ld4(x + base + down + c);
        float4 ga, gb, gd, ge;
        route(g.x, m.x, a.x, b.x, d.x, e.x, ga.x, gb.x, gd.x, ge.x);
        route(g.y, m.y, a.y, b.y, d.y, e.y, ga.y, gb.y, gd.y, ge.y);
        route(g.z, m.z, a.z, b.z, d.z, e.z, ga.z, gb.z, gd.z, ge.z);
        route(g.w, m.w, a.w, b.w, d.w, e.w, ga.w, gb.w, gd.w, ge.w);
        st4(dx + base, ga), st4(dx + base + c, gb), st4(dx + base + down, gd), st4(dx + base + down + c, ge);
    } else {
        st4(dx + base, z);  // (2 oh < h and 2 ow < w by construction of the ceil grid)
        if (has_r) st4(dx + base + c, z);
        if (has_d) st4(dx + base + down, z);
        if (has_r && has_d) st4(dx + base + down + c, z);
    }
}

}  // namespace

extern "C" {

size_t movae_vgg_prep_ws_bytes(int g) { return MOVAE_WS_HEADER_BYTES + (size_t)(g > 0 ? g : 0) * PREP_MAX_NB * sizeof(int); }

int movae_vgg_prep_fwd(int g, const float* const* x, float* const* y, int* flags, size_t n, void* ws, size_t ws_bytes,
                       movae_stream_t stream) {
    MOVAE_CHECK_ARG(g >= 1 && g <= PREP_MAX_G, "movae_vgg_prep_fwd: 1 .. %d tensors per call (got %d)", PREP_MAX_G, g);
    MOVAE_CHECK_ARG(x && y && flags && n > 0 && n % 3 == 0, "movae_vgg_prep_fwd: bad argument (n must be a multiple of the 3 channels)");
    MOVAE_CHECK_ARG(ws && ws_bytes >= movae_vgg_prep_ws_bytes(g), "movae_vgg_prep_fwd: workspace too small");
    MOVAE_WS_SCRATCH(ws, ws_bytes);
    PrepArgs a{};
    a.vec = 1;
    for (int i = 0; i < g; ++i) {
        MOVAE_CHECK_ARG(x[i] && y[i], "movae_vgg_prep_fwd: null tensor %d", i);
        a.x[i] = x[i], a.y[i] = y[i];
        a.vec &= aligned16(x[i]) && aligned16(y[i]);
    }
    a.flags = flags, a.part = static_cast<int*>(ws), a.n = (long)n;
    const int nb = prep_blocks(n);
    hipLaunchKernelGGL(prep_flag_k, dim3(nb, g), dim3(256), 0, (hipStream_t)stream, a);
    MOVAE_CHECK_LAUNCH("vgg_prep_flag");
    hipLaunchKernelGGL(prep_fwd_k, dim3(nb, g), dim3(256), 0, (hipStream_t)stream, a);
    MOVAE_CHECK_LAUNCH("vgg_prep_fwd");
    return MOVAE_OK;
}

int movae_vgg_prep_bwd(int g, const float* const* dy, const float* const* x, const int* flags, float* const* dx, size_t n,
                       movae_stream_t stream) {
    MOVAE_CHECK_ARG(g >= 1 && g <= PREP_MAX_G, "movae_vgg_prep_bwd: 1 .. %d tensors per call (got %d)", PREP_MAX_G, g);
    MOVAE_CHECK_ARG(dy && x && flags && dx && n > 0 && n % 3 == 0, "movae_vgg_prep_bwd: bad argument");
    PrepBwdArgs a{};
    a.vec = 1;
    int live = 0;
    for (int i = 0; i < g; ++i) {
        if (!dy[i]) continue;  // no cotangent for this member: nothing is written for it
        MOVAE_CHECK_ARG(x[i] && dx[i], "movae_vgg_prep_bwd: tensor %d has a cotangent but no x / dx", i);
        a.dy[live] = dy[i], a.x[live] = x[i], a.dx[live] = dx[i], a.slot[live] = i;
        a.vec &= aligned16(dy[i]) && aligned16(x[i]) && aligned16(dx[i]);
        ++live;
    }
    MOVAE_CHECK_ARG(live > 0, "movae_vgg_prep_bwd: no cotangent");
    a.flags = flags, a.n = (long)n;
    hipLaunchKernelGGL(prep_bwd_k, dim3(prep_blocks(n), live), dim3(256), 0, (hipStream_t)stream, a);
    MOVAE_CHECK_LAUNCH("vgg_prep_bwd");
    return MOVAE_OK;
}

static int pool_check(const char* who, const void* p0, const void* p1, const void* p2, const void* p3, int n, int h, int w, int c) {
    MOVAE_CHECK_ARG(n > 0 && h >= 2 && w >= 2 && c > 0, "%s: bad geometry %dx%dx%dx%d", who, n, h, w, c);
    MOVAE_CHECK_ARG(c % 4 == 0, "%s: the channel count must be a multiple of 4 (got %d)", who, c);
    MOVAE_CHECK_ARG(aligned16(p0) && aligned16(p1) && aligned16(p2) && aligned16(p3), "%s: tensors must be 16-byte aligned", who);
    return MOVAE_OK;
}

int movae_maxpool2x2_fwd(const float* x, float* y, int n, int h, int w, int c, movae_stream_t stream) {
    MOVAE_CHECK_ARG(x && y, "movae_maxpool2x2_fwd: bad argument");
    if (int rc = pool_check("movae_maxpool2x2_fwd", x, y, nullptr, nullptr, n, h, w, c)) return rc;
    const int ho = h / 2, wo = w / 2;
    const long total = (long)n * ho * wo * (c / 4);
    hipLaunchKernelGGL(maxpool_fwd_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, total, h, w, c, ho, wo);
    MOVAE_CHECK_LAUNCH("maxpool2x2_fwd");
    return MOVAE_OK;
}

int movae_maxpool2x2_bwd(const float* dy, const float* x, const float* y, float* dx, int n, int h, int w, int c, movae_stream_t stream) {
    MOVAE_CHECK_ARG(dy && x && y && dx, "movae_maxpool2x2_bwd: bad argument");
    if (int rc = pool_check("movae_maxpool2x2_bwd", dy, x, y, dx, n, h, w, c)) return rc;
    const int ho = h / 2, wo = w / 2, hc = (h + 1) / 2, wc = (w + 1) / 2;
    const long total = (long)n * hc * wc * (c / 4);
    hipLaunchKernelGGL(maxpool_bwd_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, x, y, dx, total, h, w, c,
                       ho, wo, hc, wc);
    MOVAE_CHECK_LAUNCH("maxpool2x2_bwd");
    return MOVAE_OK;
}

}  // extern "C"
