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
//
// The PixelSNAIL prior's step (prior_snail_sample_step_k, further down) is built from the same stages plus causal attention over a
// cache of every earlier position's K and V rows.
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

// The matrix that runs after the current one: its first rows are prefetched while the current one is reduced.
struct PsNext {
    const float* W;
    int R, Cp;
};

// ---- conv_in (mask A): the causal taps of h0, zero outside the grid -> xres [C][PS_S]; leaves pf = the first rows of `next` ----
__device__ __forceinline__ void ps_conv_in(const float* __restrict__ Wm, const float* __restrict__ h0, const PsDims& d, long b0, int pi, int pj,
                                           float* x, float* part, float* xres, const PsNext next, PsRows& pf) {
    const int t = threadIdx.x, B = d.B, H = d.H, W = d.W, D0 = d.D0, C = d.C, ks = d.ks, Cp = ps_pad4(C);
    const int half = ks / 2, T = ps_taps_in(ks), R = T * D0;
    ps_prefetch(Wm, R, Cp, pf);
    for (int idx = t; idx < R * PS_S; idx += PS_NT) {
        const int s = idx % PS_S, r = idx / PS_S, tap = r / D0, c = r - tap * D0;
        const int y = pi + tap / ks - half, xx = pj + tap % ks - half;
        float v = 0.f;
        if (b0 + s < B && y >= 0 && xx >= 0 && xx < W) v = h0[(((size_t)(b0 + s) * H + y) * W + xx) * D0 + c];
        x[idx] = v;
    }
    __syncthreads();
    ps_matvec(Wm, R, Cp, x, part, pf);
    ps_prefetch(next.W, next.R, next.Cp, pf);
    __syncthreads();
    for (int idx = t; idx < C * PS_S; idx += PS_NT) {
        const int s = idx % PS_S, co = idx / PS_S;
        xres[idx] = ps_out(part, Wm + (size_t)R * Cp, R, Cp, s, co);
    }
    __syncthreads();
}

// ---- one GatedResBlock on xres, over its conv1 cache A [B,H,W,C/2]; pf = the first rows of its conv1 on entry, of `next` on exit ----
__device__ __forceinline__ void ps_gated_block(const float* __restrict__ Wb, const PsPack& pk, float* __restrict__ A, const PsDims& d, long b0,
                                               int pi, int pj, float* x, float* part, float* xres, const PsNext next, PsRows& pf) {
    const int t = threadIdx.x, B = d.B, H = d.H, W = d.W, C = d.C, Ch = d.C / 2, Cp = ps_pad4(C), Chp = ps_pad4(Ch);
    const size_t pix = (size_t)pi * W + pj, HW = (size_t)H * W;
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
    ps_prefetch(next.W, next.R, next.Cp, pf);
    __syncthreads();
    for (int idx = t; idx < C * PS_S; idx += PS_NT) {
        const int s = idx % PS_S, co = idx / PS_S;
        const float* bias = Wb + pk.gf + (size_t)Ch * 2 * Cp;
        const float g = ps_out(part, bias, Ch, 2 * Cp, s, co), f = ps_out(part, bias, Ch, 2 * Cp, s, Cp + co);
        xres[idx] += (1.f / (1.f + expf(-g))) * tanhf(f);
    }
    __syncthreads();
}

// ---- head: relu, 1x1 C -> C, relu, 1x1 C -> K on xres (pf = the first rows of head conv 1), then the draw ----
__device__ __forceinline__ void ps_head_draw(const float* __restrict__ wp, const PsPack& pk, const PsDims& d, float* __restrict__ h0,
                                             int64_t* __restrict__ codes, const int64_t* __restrict__ forced,
                                             const float* __restrict__ uniforms, float* __restrict__ logits_out, long b0, size_t pix, float* x,
                                             float* part, const float* xres, PsRows& pf, float inv_temp, unsigned long long seed,
                                             unsigned long long draw, unsigned long long sample_base) {
    const int t = threadIdx.x, B = d.B, D0 = d.D0, C = d.C, K = d.K, Cp = ps_pad4(C), Kp = ps_pad4(K);
    const size_t HW = (size_t)d.H * d.W;
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

    const int C = d.C, Ch = d.C / 2, Cp = ps_pad4(C), Chp = ps_pad4(Ch);
    const long b0 = (long)blockIdx.x * PS_S;  // first sample of this workgroup; slots past the batch compute on zeros, store nothing
    const PsPack pk = ps_pack(d);
    const size_t pix = (size_t)pi * d.W + pj, HW = (size_t)d.H * d.W;
    const float* const Wblk = wp + pk.blocks;
    const PsNext head{wp + pk.head1, C, Cp};
    PsRows pf;  // the first rows of the layer that runs next

    ps_conv_in(wp + pk.conv_in, h0, d, b0, pi, pj, x, part, xres, d.L > 0 ? PsNext{Wblk + pk.conv1, C, Chp} : head, pf);
    for (int l = 0; l < d.L; ++l) {
        const float* Wb = Wblk + (size_t)l * pk.block_stride;
        ps_gated_block(Wb, pk, ac + (size_t)l * d.B * HW * Ch, d, b0, pi, pj, x, part, xres,
                       l + 1 < d.L ? PsNext{Wb + pk.block_stride + pk.conv1, C, Chp} : head, pf);
    }
    ps_head_draw(wp, pk, d, h0, codes, forced, uniforms, logits_out, b0, pix, x, part, xres, pf, inv_temp, seed, draw, sample_base);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// PixelSNAIL (models/pixelcnn_prior.py PixelSNAIL; reference :95-259).  The same step with NB PixelSNAILBlocks between conv_in and
// the head: NR gated blocks each (their conv1 caches indexed over all NB * NR gated blocks), then causal attention of the current
// position over the K / V rows of every position up to and including it, kv [NB][B][H*W][2P] (K in columns 0 .. P - 1, V in
// P .. 2P - 1, P = heads * hd), out_proj, out_conv over [r ++ attention] and the two residual adds.  The block's input stays in a
// second LDS buffer.
//
// Attention of one (sample, head) runs in one wave: a group of G = 1, 2 or 4 lanes (16 head channels per lane) owns the keys
// t = group, group + 64 / G, ... in ascending order and keeps an online softmax (m, l, o[hd]) of them; the 64 / G partials are merged
// by an xor butterfly (distances 32, 16, ..., G, the lower group's partial first), so every group ends with the same value.  The
// (sample, head) pairs go round the waves; none of this depends on the slot, the workgroup or the batch.
struct PnDims {
    PsDims g;  // g.L = NB * NR gated blocks in all
    int NB, NR, heads, hd;
};

struct PnPack {
    PsPack g;                         // conv_in, the gated block's sections, head1 / head2 / emb / total of the whole buffer
    size_t qkv, proj, outc, stride;  // relative to a PixelSNAILBlock: its NR gated blocks come first
};

__host__ __device__ inline PnPack pn_pack(const PnDims& d) {
    const size_t C = d.g.C, Cp = ps_pad4(d.g.C), P = (size_t)d.heads * d.hd, Pp = ps_pad4((int)P), Kp = ps_pad4(d.g.K);
    PnPack p;
    p.g = ps_pack(d.g);
    p.qkv = (size_t)d.NR * p.g.block_stride;
    p.proj = p.qkv + (C + 1) * 3 * Pp;
    p.outc = p.proj + (P + 1) * Cp;
    p.stride = p.outc + (2 * C + 1) * Cp;
    p.g.head1 = p.g.blocks + (size_t)d.NB * p.stride;
    p.g.head2 = p.g.head1 + (C + 1) * Cp;
    p.g.emb = p.g.head2 + (C + 1) * Kp;
    p.g.total = p.g.emb + (size_t)d.g.K * d.g.E;
    return p;
}

// LDS floats of x: what the PixelCNN layers need, out_conv's input [2C][PS_S] and out_proj's [P][PS_S]
__host__ __device__ inline size_t pn_x_floats(const PnDims& d) {
    const size_t a = ps_x_floats(d.g), r1 = 2 * (size_t)d.g.C, r2 = (size_t)d.heads * d.hd;
    const size_t b = (((r1 > r2 ? r1 : r2) * PS_S) + 3) & ~(size_t)3;
    return a > b ? a : b;
}
__host__ __device__ inline size_t pn_lds_floats(const PnDims& d) {  // x | part | xres | xblk | q [PS_S][pad4(P)]
    return pn_x_floats(d) + PS_PART_FLOATS + 2 * (size_t)ps_pad4(d.g.C) * PS_S + (size_t)PS_S * ps_pad4(d.heads * d.hd);
}

constexpr int PN_DL = 16;  // head channels per lane

// channels c .. c + 3 of the n channels a lane owns of a K or V row, zero past them
template <bool V4>
__device__ __forceinline__ f32x4 pn_row4(const float* __restrict__ row, int c, int n) {
    if (V4) return *reinterpret_cast<const f32x4*>(row + c);
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = c + e < n ? row[c + e] : 0.f;
    return r;
}

// One (sample, head) in one wave.  kvs = the head's K row of raster index 0 (row t lies t * ld floats further, its V row P floats
// behind it), qh = the head's q in LDS; writes o[d] / l to xo[d * ostride], d < hd.  A group of G = 1 << lg consecutive lanes,
// hd <= PN_DL * G, shares a key: lane g of it owns the channels PN_DL * g .. of the score and of o.  V4: hd % 4 == 0, so what a
// lane reads of a row is 16-byte aligned.
template <bool V4>
__device__ __forceinline__ void pn_attend(const float* __restrict__ kvs, const float* qh, int hd, int lg, int P, size_t ld, size_t pix,
                                          float scale, float* xo, int ostride) {
    const int lane = threadIdx.x & 63, G = 1 << lg, g = lane & (G - 1), c0 = PN_DL * g;
    const int n = hd - c0 < PN_DL ? hd - c0 : PN_DL;  // (<= 0: the lane owns no channel)
    float m = -INFINITY, l = 0.f, o[PN_DL];
#pragma unroll
    for (int dd = 0; dd < PN_DL; ++dd) o[dd] = 0.f;
    // (keeping four keys' rows in flight per lane instead of one was measured and bought nothing: DESIGN.md 3.20)
#pragma unroll 1
    for (size_t t = lane >> lg; t <= pix; t += 64 >> lg) {
        const float* __restrict__ kr = kvs + t * ld + c0;
        const float* __restrict__ vr = kr + P;
        f32x4 k4[PN_DL / 4], v4[PN_DL / 4];
#pragma unroll
        for (int c4 = 0; c4 < PN_DL / 4; ++c4) {
            k4[c4] = v4[c4] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (4 * c4 < n) k4[c4] = pn_row4<V4>(kr, 4 * c4, n), v4[c4] = pn_row4<V4>(vr, 4 * c4, n);
        }
        float sc = 0.f;
#pragma unroll
        for (int dd = 0; dd < PN_DL; ++dd)
            if (dd < n) sc += qh[c0 + dd] * k4[dd / 4][dd % 4];
        for (int off = 1; off < G; off <<= 1) sc += __shfl_xor(sc, off, 64);  // (a + b on both sides: the group agrees bitwise)
        sc *= scale;
        const float mn = fmaxf(m, sc), a = expf(m - mn), p = expf(sc - mn);  // (m = -inf before the first key: a = 0)
        l = l * a + p;
#pragma unroll
        for (int dd = 0; dd < PN_DL; ++dd) o[dd] = o[dd] * a + p * v4[dd / 4][dd % 4];
        m = mn;
    }
    // the 64 / G partials, merged by an xor butterfly over the groups; the lower group's partial is the first operand on both sides
    for (int off = 32; off >= G; off >>= 1) {
        const bool lo = (lane & off) == 0;
        const float m2 = __shfl_xor(m, off, 64), l2 = __shfl_xor(l, off, 64);
        const float ma = lo ? m : m2, mb = lo ? m2 : m, mn = fmaxf(ma, mb);
        const float a = ma == -INFINITY ? 0.f : expf(ma - mn), b = mb == -INFINITY ? 0.f : expf(mb - mn);
        l = (lo ? l : l2) * a + (lo ? l2 : l) * b;
#pragma unroll
        for (int dd = 0; dd < PN_DL; ++dd) {
            const float o2 = __shfl_xor(o[dd], off, 64);
            o[dd] = (lo ? o[dd] : o2) * a + (lo ? o2 : o[dd]) * b;
        }
        m = mn;
    }
    if (lane < G) {
#pragma unroll
        for (int dd = 0; dd < PN_DL; ++dd)
            if (dd < n) xo[(size_t)(c0 + dd) * ostride] = o[dd] / l;
    }
}

__global__ __launch_bounds__(PS_NT) void prior_snail_sample_step_k(const float* __restrict__ wp, float* __restrict__ h0, float* __restrict__ ac,
                                                                  float* __restrict__ kv, int64_t* __restrict__ codes,
                                                                  const int64_t* __restrict__ forced, const float* __restrict__ uniforms,
                                                                  float* __restrict__ logits_out, PnDims dn, int pi, int pj, float inv_temp,
                                                                  unsigned long long seed, unsigned long long draw,
                                                                  unsigned long long sample_base) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const PsDims& d = dn.g;
    const int t = threadIdx.x, B = d.B, C = d.C, Ch = d.C / 2, Cp = ps_pad4(C), Chp = ps_pad4(Ch);
    const int heads = dn.heads, hd = dn.hd, P = heads * hd, Pp = ps_pad4(P);
    float* const x = lds;
    float* const part = x + pn_x_floats(dn);
    float* const xres = part + PS_PART_FLOATS;      // the stream through the gated blocks: r
    float* const xblk = xres + (size_t)Cp * PS_S;   // the PixelSNAILBlock's input
    float* const qb = xblk + (size_t)Cp * PS_S;     // q of this position [PS_S][Pp]

    const long b0 = (long)blockIdx.x * PS_S;
    const PnPack pk = pn_pack(dn);
    const size_t pix = (size_t)pi * d.W + pj, HW = (size_t)d.H * d.W;
    const float* const Wblk = wp + pk.g.blocks;
    const PsNext head{wp + pk.g.head1, C, Cp};
    // the first matrix of PixelSNAILBlock nb: its first gated block's conv1, or q ++ k ++ v where it has no gated block
    auto first_of = [&](int nb) {
        const float* Wsb = Wblk + (size_t)nb * pk.stride;
        return dn.NR > 0 ? PsNext{Wsb + pk.g.conv1, C, Chp} : PsNext{Wsb + pk.qkv, C, 3 * Pp};
    };
    const float scale = 1.f / sqrtf((float)hd);
    PsRows pf;

    ps_conv_in(wp + pk.g.conv_in, h0, d, b0, pi, pj, x, part, xres, dn.NB > 0 ? first_of(0) : head, pf);
    for (int idx = t; idx < C * PS_S; idx += PS_NT) xblk[idx] = xres[idx];

    for (int nb = 0; nb < dn.NB; ++nb) {
        const float* Wsb = Wblk + (size_t)nb * pk.stride;
        // The widths pass through an opaque register: every block works its thread offsets and loop bounds out again.  Hoisted out
        // of this loop they would stay live across every layer of the block, which costs more registers than the kernel has.
        int Cv = d.C, hdv = dn.hd;
        asm volatile("" : "+s"(Cv), "+s"(hdv));
        PsDims dl = d;
        dl.C = Cv;
        const int C = Cv, Ch = C / 2, Cp = ps_pad4(C), Chp = ps_pad4(Ch), hd = hdv, P = heads * hd, Pp = ps_pad4(P);
        for (int g = 0; g < dn.NR; ++g) {
            const float* Wb = Wsb + (size_t)g * pk.g.block_stride;
            ps_gated_block(Wb, pk.g, ac + (size_t)(nb * dn.NR + g) * B * HW * Ch, dl, b0, pi, pj, x, part, xres,
                           g + 1 < dn.NR ? PsNext{Wb + pk.g.block_stride + pk.g.conv1, C, Chp} : PsNext{Wsb + pk.qkv, C, 3 * Pp}, pf);
        }
        // q ++ k ++ v = r W + b: q to LDS, k and v to the cache at this raster index
        ps_matvec(Wsb + pk.qkv, C, 3 * Pp, xres, part, pf);
        __syncthreads();
        float* const kvb = kv + (size_t)nb * B * HW * 2 * P;
        for (int idx = t; idx < 3 * P * PS_S; idx += PS_NT) {
            const int s = idx % PS_S, co = idx / PS_S, which = co / P, c = co - which * P;
            const float v = ps_out(part, Wsb + pk.qkv + (size_t)C * 3 * Pp, C, 3 * Pp, s, which * Pp + c);
            if (which == 0) qb[(size_t)s * Pp + c] = v;
            else if (b0 + s < B) kvb[((size_t)(b0 + s) * HW + pix) * 2 * P + (size_t)(which - 1) * P + c] = v;
        }
        __syncthreads();  // (this position's k and v are read back from the cache below)
        // attention of every (sample, head) over the keys 0 .. pix, written in the reference's channel order d * heads + h
        for (int p = t >> 6; p < PS_S * heads; p += PS_NT / 64) {
            const int s = p / heads, h = p - s * heads;
            float* xo = x + (size_t)h * PS_S + s;
            const int ostride = heads * PS_S;
            if (b0 + s >= B) {
                for (int dd = t & 63; dd < hd; dd += 64) xo[(size_t)dd * ostride] = 0.f;
                continue;
            }
            const float* kvs = kvb + (size_t)(b0 + s) * HW * 2 * P + (size_t)h * hd;
            const float* qh = qb + (size_t)s * Pp + (size_t)h * hd;
            const size_t ld = 2 * (size_t)P;
            const int lg = hd <= PN_DL ? 0 : (hd <= 2 * PN_DL ? 1 : 2);
            if ((hd & 3) == 0) pn_attend<true>(kvs, qh, hd, lg, P, ld, pix, scale, xo, ostride);
            else pn_attend<false>(kvs, qh, hd, lg, P, ld, pix, scale, xo, ostride);
        }
        ps_prefetch(Wsb + pk.proj, P, Cp, pf);
        __syncthreads();
        // out_proj, then out_conv over [r ++ attention]
        ps_matvec(Wsb + pk.proj, P, Cp, x, part, pf);
        ps_prefetch(Wsb + pk.outc, 2 * C, Cp, pf);
        __syncthreads();
        for (int idx = t; idx < C * PS_S; idx += PS_NT) {
            const int s = idx % PS_S, co = idx / PS_S;
            x[(size_t)(C + co) * PS_S + s] = ps_out(part, Wsb + pk.proj + (size_t)P * Cp, P, Cp, s, co);
            x[idx] = xres[idx];
        }
        __syncthreads();
        ps_matvec(Wsb + pk.outc, 2 * C, Cp, x, part, pf);
        const PsNext next = nb + 1 < dn.NB ? first_of(nb + 1) : head;
        ps_prefetch(next.W, next.R, next.Cp, pf);
        __syncthreads();
        // x + block(x), block(x) = out_conv(...) + r
        for (int idx = t; idx < C * PS_S; idx += PS_NT) {
            const int s = idx % PS_S, co = idx / PS_S;
            const float v = xblk[idx] + (ps_out(part, Wsb + pk.outc + (size_t)2 * C * Cp, 2 * C, Cp, s, co) + xres[idx]);
            xblk[idx] = v;
            xres[idx] = v;
        }
        __syncthreads();
    }
    ps_head_draw(wp, pk.g, d, h0, codes, forced, uniforms, logits_out, b0, pix, x, part, xres, pf, inv_temp, seed, draw, sample_base);
}

bool ps_supported(const PsDims& d) {
    return d.B >= 1 && d.H >= 1 && d.W >= 1 && d.C >= 2 && d.C % 2 == 0 && d.C <= 256 && d.D0 >= 1 && d.D0 <= 256 && d.E >= 1 && d.E <= d.D0 &&
           d.K >= 1 && d.K <= 2048 && d.ks >= 1 && d.ks % 2 == 1 && d.ks <= 7 && d.L >= 0;
}

bool pn_supported(const PnDims& d) {
    return d.NB >= 0 && d.NR >= 0 && d.NB <= 4096 && d.NR <= 4096 && d.g.L == d.NB * d.NR && ps_supported(d.g) && d.g.E + 2 <= d.g.D0 &&
           d.heads >= 1 && d.hd >= 1 && d.hd <= 64 && d.heads <= 256 && d.heads * d.hd <= 256;
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

size_t movae_prior_snail_sample_pack_floats(int D0, int E, int C, int NB, int NR, int heads, int hd, int K, int ks) {
    if (NB < 0 || NR < 0 || NB > 4096 || NR > 4096) return 0;
    const PnDims d{{1, 1, 1, D0, E, C, NB * NR, K, ks}, NB, NR, heads, hd};
    return pn_supported(d) ? pn_pack(d).g.total : 0;
}

int movae_prior_snail_sample_step(const float* wpack, size_t wpack_floats, float* h0, float* acache, float* kvcache, int64_t* codes,
                                  const int64_t* forced, const float* uniforms, float* logits_out, int B, int H, int W, int D0, int E, int C,
                                  int NB, int NR, int heads, int hd, int K, int ks, int i, int j, float inv_temperature,
                                  unsigned long long seed, unsigned long long draw, unsigned long long sample_base, movae_stream_t stream) {
    MOVAE_CHECK_ARG(NB >= 0 && NR >= 0 && NB <= 4096 && NR <= 4096, "movae_prior_snail_sample_step: 0 <= blocks, gated blocks per block <= 4096");
    const PnDims d{{B, H, W, D0, E, C, NB * NR, K, ks}, NB, NR, heads, hd};
    MOVAE_CHECK_ARG(pn_supported(d),
                    "movae_prior_snail_sample_step: unsupported shape (hidden even <= 256, E + 2 <= D0 <= 256, K <= 2048, odd kernel <= 7, "
                    "head_dim <= 64, heads * head_dim <= 256)");
    MOVAE_CHECK_ARG(wpack && h0 && codes && (acache || NB * NR == 0) && (kvcache || NB == 0), "movae_prior_snail_sample_step: null buffer");
    MOVAE_CHECK_ARG(i >= 0 && i < H && j >= 0 && j < W, "movae_prior_snail_sample_step: position outside the grid");
    MOVAE_CHECK_ARG(wpack_floats == pn_pack(d).g.total, "movae_prior_snail_sample_step: packed weights have %zu floats, the layout has %zu",
                    wpack_floats, pn_pack(d).g.total);
    MOVAE_CHECK_ARG((reinterpret_cast<uintptr_t>(wpack) & 15) == 0 && (reinterpret_cast<uintptr_t>(kvcache) & 15) == 0,
                    "movae_prior_snail_sample_step: packed weights and the K/V cache must be 16-byte aligned");
    MOVAE_CHECK_ARG((unsigned long long)H * W < (1ull << 32) && sample_base + (unsigned long long)B < (1ull << 32),
                    "movae_prior_snail_sample_step: sample and raster indices are 32-bit Philox counter words");
    const size_t lds_bytes = pn_lds_floats(d) * sizeof(float);
    if (lds_bytes > (size_t)(160 << 10)) {
        movae_set_error("movae_prior_snail_sample_step: needs %zu bytes of LDS, a workgroup has 160 KiB", lds_bytes);
        return MOVAE_EUNSUPPORTED;
    }
    static size_t lds_allowed = 48 << 10;
    if (lds_bytes > lds_allowed) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(prior_snail_sample_step_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_bytes) != hipSuccess) {
            (void)hipGetLastError();
            movae_set_error("movae_prior_snail_sample_step: %zu bytes of LDS refused", lds_bytes);
            return MOVAE_EUNSUPPORTED;
        }
        lds_allowed = lds_bytes;
    }
    hipLaunchKernelGGL(prior_snail_sample_step_k, dim3((unsigned)((B + PS_S - 1) / PS_S)), dim3(PS_NT), lds_bytes, (hipStream_t)stream, wpack,
                       h0, acache, kvcache, codes, forced, uniforms, logits_out, d, i, j, inv_temperature, seed, draw, sample_base);
    MOVAE_CHECK_LAUNCH("prior_snail_sample_step");
    return MOVAE_OK;
}

}  // extern "C"
