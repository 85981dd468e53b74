// Cached ancestral sampling for the PixelCNN prior (models/pixelcnn_prior.py PixelCNN.sample; reference :323-349): one launch
// computes raster position (i, j) of every sample of the batch -- conv_in over the causal taps of the cached input grid, the
// gated residual blocks over their cached conv1 outputs, the head, and the categorical draw -- instead of a full-grid forward.
//
// The network is causal: what a layer needs at (i, j) was computed at earlier raster positions and never changes.  Only h0
// (embedding ++ condition, [B,H,W,D0]) and the blocks' conv1 outputs A_l ([L][B,H,W,C/2]) live in HBM; the residual stream of the
// current position stays in LDS.  A workgroup owns PS_S consecutive samples; workgroups never talk to each other.
//
// Every layer of one position is a matrix-vector product y[co] = sum_r W[r][co] x[r] per sample.  Weights are packed
// [r][co padded to 4] (sampling.py: pack_weights; r = tap * cin + ci over the causal taps only), so a wave reads 1 KiB of
// consecutive weights per load: thread t owns the four output channels 4 * (t % Q) .. of the rows r = t / Q, t / Q + nsl, ...
// (Q = co_pad / 4, nsl = PS_NT / Q), each weight load feeds one FMA per owned sample with x broadcast from LDS, and the nsl
// partial sums of an output are added in slice order.  The order of a sample's arithmetic depends on the layer's shape alone,
// never on the slot or the workgroup the sample sits in.
#include "common.h"

namespace {

constexpr int PS_NT = 512;  // threads per workgroup: 4 * PS_NT >= the widest padded output (K <= 2048, 2 * C <= 512)
constexpr int PS_S = 4;     // samples per workgroup

struct PsDims {
    int B, H, W, D0, E, C, L, K, ks;
};

__host__ __device__ inline int ps_pad4(int n) { return (n + 3) & ~3; }
__host__ __device__ inline int ps_taps_in(int ks) { return (ks / 2) * ks + ks / 2; }

// float offsets of the packed buffer's sections (the layout sampling.py writes)
struct PsPack {
    size_t conv_in, blocks, block_stride, conv1, conv2, gf, head1, head2, emb, total;  // conv1 / conv2 / gf relative to a block
};

__host__ __device__ inline PsPack ps_pack(const PsDims& d) {
    const size_t Cp = ps_pad4(d.C), Ch = d.C / 2, Chp = ps_pad4(d.C / 2), Kp = ps_pad4(d.K);
    PsPack p;
    p.conv_in = 0;
    p.blocks = ((size_t)ps_taps_in(d.ks) * d.D0 + 1) * Cp;
    p.conv1 = 0;
    p.conv2 = ((size_t)d.C + 1) * Chp;
    p.gf = p.conv2 + (5 * Ch + 1) * Chp;
    p.block_stride = p.gf + (Ch + 1) * 2 * Cp;
    p.head1 = p.blocks + (size_t)d.L * p.block_stride;
    p.head2 = p.head1 + ((size_t)d.C + 1) * Cp;
    p.emb = p.head2 + ((size_t)d.C + 1) * Kp;
    p.total = p.emb + (size_t)d.K * d.E;
    return p;
}

// LDS floats: x (layer inputs [r][PS_S], later the logits [PS_S][Kp]) | part (slice partials) | xres (residual stream [C][PS_S])
__host__ __device__ inline size_t ps_x_floats(const PsDims& d) {
    size_t r = (size_t)ps_taps_in(d.ks) * d.D0;
    const size_t r2 = 5 * (size_t)(d.C / 2), r3 = d.C, r4 = ps_pad4(d.K);
    r = r > r2 ? r : r2;
    r = r > r3 ? r : r3;
    r = r > r4 ? r : r4;
    return (r * PS_S + 3) & ~(size_t)3;
}
constexpr size_t PS_PART_FLOATS = (size_t)PS_S * 4 * PS_NT;

// A thread's first PS_PF weight rows of a layer.  Weight addresses depend on no activation, so a layer's first rows are loaded
// while the layer before it is still being reduced: the load latency hides behind the barriers and the LDS reduce.
constexpr int PS_PF = 8;
struct PsRows {
    f32x4 w[PS_PF];
};

__device__ __forceinline__ void ps_prefetch(const float* __restrict__ Wm, int R, int Cp, PsRows& pf) {
    const int Q = Cp >> 2, nsl = PS_NT / Q, t = threadIdx.x, q = t % Q, sl = t / Q;
    const f32x4* __restrict__ W4 = reinterpret_cast<const f32x4*>(Wm);
#pragma unroll
    for (int u = 0; u < PS_PF; ++u) {
        const int r = sl + u * nsl;
        pf.w[u] = sl < nsl && r < R ? W4[(size_t)r * Q + q] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// part[(sl * PS_S + s) * Cp + co] = sum over the rows of slice sl of W[r][co] * x[r][s]   (Cp / 4 <= PS_NT); pf = ps_prefetch of
// the same matrix.  The rows are added in ascending order whether they were prefetched or not.
__device__ __forceinline__ void ps_matvec(const float* __restrict__ Wm, int R, int Cp, const float* x, float* part, const PsRows& pf) {
    const int Q = Cp >> 2, nsl = PS_NT / Q, t = threadIdx.x, q = t % Q, sl = t / Q;
    if (sl >= nsl) return;
    const f32x4* __restrict__ W4 = reinterpret_cast<const f32x4*>(Wm);
    f32x4 acc[PS_S];
#pragma unroll
    for (int s = 0; s < PS_S; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < PS_PF; ++u) {
        const int r = sl + u * nsl;
        if (r < R) {
            const f32x4 xs = *reinterpret_cast<const f32x4*>(x + (size_t)r * PS_S);
#pragma unroll
            for (int s = 0; s < PS_S; ++s) acc[s] += pf.w[u] * xs[s];
        }
    }
#pragma unroll 8
    for (int r = sl + PS_PF * nsl; r < R; r += nsl) {
        const f32x4 w = W4[(size_t)r * Q + q];
        const f32x4 xs = *reinterpret_cast<const f32x4*>(x + (size_t)r * PS_S);
#pragma unroll
        for (int s = 0; s < PS_S; ++s) acc[s] += w * xs[s];
    }
#pragma unroll
    for (int s = 0; s < PS_S; ++s) *reinterpret_cast<f32x4*>(part + (size_t)(sl * PS_S + s) * Cp + 4 * q) = acc[s];
}

// the finished output (s, co) of the last ps_matvec over R rows: slice partials in slice order, then the bias
__device__ __forceinline__ float ps_out(const float* part, const float* __restrict__ bias, int R, int Cp, int s, int co) {
    int nsl = PS_NT / (Cp >> 2);
    nsl = nsl < R ? nsl : R;  // (slices past the last row hold zeros)
    float v = 0.f;
    for (int sl = 0; sl < nsl; ++sl) v += part[(size_t)(sl * PS_S + s) * Cp + co];
    return v + bias[co];
}

__global__ __launch_bounds__(PS_NT) void prior_sample_step_k(const float* __restrict__ wp, float* __restrict__ h0, float* __restrict__ ac,
                                                            int64_t* __restrict__ codes, const int64_t* __restrict__ forced,
                                                            const float* __restrict__ uniforms, float* __restrict__ logits_out, PsDims d,
                                                            int pi, int pj, float inv_temp, unsigned long long seed,
                                                            unsigned long long draw, unsigned long long sample_base) {
    static_assert(PS_S == 4, "ps_matvec reads the PS_S inputs of a row as one f32x4");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const x = lds;
    float* const part = x + ps_x_floats(d);
    float* const xres = part + PS_PART_FLOATS;

    const int t = threadIdx.x;
    const int B = d.B, H = d.H, W = d.W, D0 = d.D0, C = d.C, Ch = d.C / 2, K = d.K, ks = d.ks;
    const int Cp = ps_pad4(C), Chp = ps_pad4(Ch), Kp = ps_pad4(K);
    const long b0 = (long)blockIdx.x * PS_S;  // first sample of this workgroup; slots past the batch compute on zeros, store nothing
    const PsPack pk = ps_pack(d);
    const size_t pix = (size_t)pi * W + pj, HW = (size_t)H * W;
    const float* const Wblk = wp + pk.blocks;
    PsRows pf;  // the first rows of the layer that runs next

    // ---- conv_in (mask A): the causal taps of h0, zero outside the grid ----
    {
        const int half = ks / 2, T = ps_taps_in(ks), R = T * D0;
        ps_prefetch(wp + pk.conv_in, R, Cp, pf);
        for (int idx = t; idx < R * PS_S; idx += PS_NT) {
            const int s = idx % PS_S, r = idx / PS_S, tap = r / D0, c = r - tap * D0;
            const int y = pi + tap / ks - half, xx = pj + tap % ks - half;
            float v = 0.f;
            if (b0 + s < B && y >= 0 && xx >= 0 && xx < W) v = h0[(((size_t)(b0 + s) * H + y) * W + xx) * D0 + c];
            x[idx] = v;
        }
        __syncthreads();
        const float* Wm = wp + pk.conv_in;
        ps_matvec(Wm, R, Cp, x, part, pf);
        if (d.L > 0) ps_prefetch(Wblk + pk.conv1, C, Chp, pf);
        else ps_prefetch(wp + pk.head1, C, Cp, pf);
        __syncthreads();
        for (int idx = t; idx < C * PS_S; idx += PS_NT) {
            const int s = idx % PS_S, co = idx / PS_S;
            xres[idx] = ps_out(part, Wm + (size_t)R * Cp, R, Cp, s, co);
        }
        __syncthreads();
    }

    // ---- gated residual blocks ----
    for (int l = 0; l < d.L; ++l) {
        const float* Wb = Wblk + (size_t)l * pk.block_stride;
        float* A = ac + (size_t)l * B * HW * Ch;
        // a = relu(conv1 x + b): cached at (i, j), and the centre tap of conv2
        ps_matvec(Wb + pk.conv1, C, Chp, xres, part, pf);
        ps_prefetch(Wb + pk.conv2, 5 * Ch, Chp, pf);
        // (meanwhile) the four earlier taps of the masked-B 3x3, from the cache
        for (int idx = t; idx < 4 * Ch * PS_S; idx += PS_NT) {
            const int s = idx % PS_S, r = idx / PS_S, tap = r / Ch, c = r - tap * Ch;
            const int y = pi + (tap < 3 ? -1 : 0), xx = pj + (tap < 3 ? tap - 1 : -1);
            float v = 0.f;
            if (b0 + s < B && y >= 0 && xx >= 0 && xx < W) v = A[(((size_t)(b0 + s) * H + y) * W + xx) * Ch + c];
            x[idx] = v;
        }
        __syncthreads();
        for (int idx = t; idx < Ch * PS_S; idx += PS_NT) {
            const int s = idx % PS_S, co = idx / PS_S;
            float v = ps_out(part, Wb + pk.conv1 + (size_t)C * Chp, C, Chp, s, co);
            v = v > 0.f ? v : 0.f;
            x[(size_t)(4 * Ch + co) * PS_S + s] = v;
            if (b0 + s < B) A[((size_t)(b0 + s) * HW + pix) * Ch + co] = v;
        }
        __syncthreads();
        // m = relu(masked-B 3x3 over A)
        ps_matvec(Wb + pk.conv2, 5 * Ch, Chp, x, part, pf);
        ps_prefetch(Wb + pk.gf, Ch, 2 * Cp, pf);
        __syncthreads();
        for (int idx = t; idx < Ch * PS_S; idx += PS_NT) {
            const int s = idx % PS_S, co = idx / PS_S;
            const float v = ps_out(part, Wb + pk.conv2 + (size_t)5 * Ch * Chp, 5 * Ch, Chp, s, co);
            x[idx] = v > 0.f ? v : 0.f;
        }
        __syncthreads();
        // x += sigmoid(conv_gate m) * tanh(conv_feature m): gate in columns 0 .. Cp - 1, feature in Cp .. 2 Cp - 1
        ps_matvec(Wb + pk.gf, Ch, 2 * Cp, x, part, pf);
        if (l + 1 < d.L) ps_prefetch(Wb + pk.block_stride + pk.conv1, C, Chp, pf);
        else ps_prefetch(wp + pk.head1, C, Cp, pf);
        __syncthreads();
        for (int idx = t; idx < C * PS_S; idx += PS_NT) {
            const int s = idx % PS_S, co = idx / PS_S;
            const float* bias = Wb + pk.gf + (size_t)Ch * 2 * Cp;
            const float g = ps_out(part, bias, Ch, 2 * Cp, s, co), f = ps_out(part, bias, Ch, 2 * Cp, s, Cp + co);
            xres[idx] += (1.f / (1.f + expf(-g))) * tanhf(f);
        }
        __syncthreads();
    }

    // ---- head: relu, 1x1 C -> C, relu, 1x1 C -> K ----
    for (int idx = t; idx < C * PS_S; idx += PS_NT) x[idx] = xres[idx] > 0.f ? xres[idx] : 0.f;
    __syncthreads();
    ps_matvec(wp + pk.head1, C, Cp, x, part, pf);
    ps_prefetch(wp + pk.head2, C, Kp, pf);
    __syncthreads();
    for (int idx = t; idx < C * PS_S; idx += PS_NT) {
        const int s = idx % PS_S, co = idx / PS_S;
        const float v = ps_out(part, wp + pk.head1 + (size_t)C * Cp, C, Cp, s, co);
        x[idx] = v > 0.f ? v : 0.f;
    }
    __syncthreads();
    ps_matvec(wp + pk.head2, C, Kp, x, part, pf);
    __syncthreads();
    float* const lg = x;  // [PS_S][Kp]: the matvec above has read x for the last time
    for (int idx = t; idx < K * PS_S; idx += PS_NT) {
        const int s = idx / K, k = idx - s * K;
        const float v = ps_out(part, wp + pk.head2 + (size_t)C * Kp, C, Kp, s, k);
        lg[(size_t)s * Kp + k] = v;
        if (logits_out && b0 + s < B) logits_out[((size_t)(b0 + s) * HW + pix) * K + k] = v;
    }
    __syncthreads();

    // ---- the draw: wave s draws sample s.  code = the smallest k with u < cdf_k of softmax(logits / T), clamped to K - 1 ----
    const int wave = t >> 6, lane = t & 63;
    if (wave >= PS_S || b0 + wave >= B) return;
    const long b = b0 + wave;
    long code;
    if (forced) {
        code = forced[(size_t)b * HW + pix];
        code = code < 0 ? 0 : (code >= K ? K - 1 : code);
    } else {
        const float* z = lg + (size_t)wave * Kp;
        float u;
        if (uniforms) {
            u = uniforms[(size_t)b * HW + pix];
        } else {
            const unsigned long long sample = sample_base + (unsigned long long)b;
            unsigned w4[4];
            philox4x32_10((unsigned)sample, (unsigned)pix, (unsigned)draw, (unsigned)(draw >> 32), (unsigned)seed, (unsigned)(seed >> 32), w4);
            u = (float)(w4[0] >> 8) * (1.f / 16777216.f);  // [0, 1), 24 bits
        }
        float m = -INFINITY;
        for (int k = lane; k < K; k += 64) m = fmaxf(m, z[k] * inv_temp);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        // lane owns the codes [k0, k1): its mass, then the masses of the lanes before it
        const int per = (K + 63) / 64, k0 = lane * per < K ? lane * per : K, k1 = k0 + per < K ? k0 + per : K;
        float mine = 0.f;
        for (int k = k0; k < k1; ++k) mine += expf(z[k] * inv_temp - m);
        float incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        const float total = __shfl(incl, 63, 64), target = u * total;
        float run = incl - mine;
        int found = K;
        for (int k = k0; k < k1; ++k) {
            run += expf(z[k] * inv_temp - m);
            if (found == K && target < run) found = k;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int other = __shfl_xor(found, o, 64);
            found = other < found ? other : found;
        }
        code = found < K ? found : K - 1;
    }
    if (lane == 0) codes[(size_t)b * HW + pix] = (int64_t)code;
    const float* e = wp + pk.emb + (size_t)code * d.E;
    float* dst = h0 + ((size_t)b * HW + pix) * D0;
    for (int c = lane; c < d.E; c += 64) dst[c] = e[c];
}

bool ps_supported(const PsDims& d) {
    return d.B >= 1 && d.H >= 1 && d.W >= 1 && d.C >= 2 && d.C % 2 == 0 && d.C <= 256 && d.D0 >= 1 && d.D0 <= 256 && d.E >= 1 && d.E <= d.D0 &&
           d.K >= 1 && d.K <= 2048 && d.ks >= 1 && d.ks % 2 == 1 && d.ks <= 7 && d.L >= 0;
}

}  // namespace

extern "C" {

size_t movae_prior_sample_pack_floats(int D0, int E, int C, int L, int K, int ks) {
    const PsDims d{1, 1, 1, D0, E, C, L, K, ks};
    return ps_supported(d) ? ps_pack(d).total : 0;
}

int movae_prior_sample_step(const float* wpack, size_t wpack_floats, float* h0, float* acache, int64_t* codes, const int64_t* forced,
                            const float* uniforms, float* logits_out, int B, int H, int W, int D0, int E, int C, int L, int K, int ks, int i,
                            int j, float inv_temperature, unsigned long long seed, unsigned long long draw, unsigned long long sample_base,
                            movae_stream_t stream) {
    const PsDims d{B, H, W, D0, E, C, L, K, ks};
    MOVAE_CHECK_ARG(ps_supported(d), "movae_prior_sample_step: unsupported shape (hidden even <= 256, D0 <= 256, K <= 2048, odd kernel <= 7)");
    MOVAE_CHECK_ARG(wpack && h0 && codes && (acache || L == 0), "movae_prior_sample_step: null buffer");
    MOVAE_CHECK_ARG(i >= 0 && i < H && j >= 0 && j < W, "movae_prior_sample_step: position outside the grid");
    MOVAE_CHECK_ARG(wpack_floats == ps_pack(d).total, "movae_prior_sample_step: packed weights have %zu floats, the layout has %zu",
                    wpack_floats, ps_pack(d).total);
    MOVAE_CHECK_ARG((reinterpret_cast<uintptr_t>(wpack) & 15) == 0, "movae_prior_sample_step: packed weights must be 16-byte aligned");
    MOVAE_CHECK_ARG((unsigned long long)H * W < (1ull << 32) && sample_base + (unsigned long long)B < (1ull << 32),
                    "movae_prior_sample_step: sample and raster indices are 32-bit Philox counter words");
    const size_t lds_bytes = (ps_x_floats(d) + PS_PART_FLOATS + (size_t)ps_pad4(C) * PS_S) * sizeof(float);
    static size_t lds_allowed = 48 << 10;
    if (lds_bytes > lds_allowed) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(prior_sample_step_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_bytes) != hipSuccess) {
            (void)hipGetLastError();
            movae_set_error("movae_prior_sample_step: %zu bytes of LDS refused", lds_bytes);
            return MOVAE_EUNSUPPORTED;
        }
        lds_allowed = lds_bytes;
    }
    hipLaunchKernelGGL(prior_sample_step_k, dim3((unsigned)((B + PS_S - 1) / PS_S)), dim3(PS_NT), lds_bytes, (hipStream_t)stream, wpack, h0,
                       acache, codes, forced, uniforms, logits_out, d, i, j, inv_temperature, seed, draw, sample_base);
    MOVAE_CHECK_LAUNCH("prior_sample_step");
    return MOVAE_OK;
}

}  // extern "C"
