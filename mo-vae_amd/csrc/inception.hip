// Forward-only inference kernels of the Inception-v3 feature stack behind rFID (reference utils/metrics.py:360-450 InceptionV3,
// :513-615 calculate_fid; the stack itself is driven from inception.py).  None of this is training code: no autograd, no fusion state,
// nothing shared with the conv dispatcher of conv_igemm.hip.
//
//   infer_conv_k<BM, BN, VEC>   implicit GEMM, M = n ho wo, N = co, K = kh kw ci, independent kernel sides and paddings, on
//                               v_mfma_f32_32x32x2_f32 (exact fp32: one rounding per product, k-ordered sum).  Both operands are
//                               k-contiguous ([pixel][tap][ci] gathered, [co][tap][ci] stored), so both live row-major [row][32 + 4]
//                               in LDS, written with one 16-byte store per 4 k and read with 16-byte reads (4 MFMA operands each;
//                               144-byte rows keep 16-lane groups conflict-free).  Lane half h consumes k = 16 h + j at step j in
//                               both operands.  One LDS stage; the next stage's global loads are issued before the MFMAs of the
//                               current one and land in LDS behind them (two barriers per 32 k).  VEC (ci % 4 == 0, aligned
//                               operands): a thread's 4 k lie inside one tap -> one 16-byte load; otherwise (the 3-channel stem,
//                               odd widths) every k is decoded and loaded on its own.  Epilogue: max(0, acc * scale[o] + shift[o])
//                               straight from the accumulators into channels coff .. of an ldy-wide output row: for one
//                               accumulator register 32 lanes write 32 consecutive floats.
//   infer_pool_k / infer_pool4_k  3x3 max (stride 2, no padding) / 3x3 average (stride 1, padding 1, / 9 always), one thread per
//                               output element (per four channels where c, the output row and the offset allow 16-byte accesses),
//                               c fastest.
//   infer_gmean_k               mean over the pixels, one thread per (image, channel).
//   inception_prep_k<FILTER>    calculate_fid's denormalize + TF.resize(299, BICUBIC, antialias) + centre crop + normalize, one
//                               thread per output pixel, NCHW in, NHWC out.  FILTER 1: the same with TF.resize's default BILINEAR
//                               (the triangle filter), calculate_inception_score's pipeline.
#include "common.h"

#include <math.h>

namespace {

constexpr int IC_BK = 32;          // k per stage
constexpr int IC_LDR = IC_BK + 4;  // floats per LDS row
constexpr int IC_OUT = 299;

struct ConvP {
    const float* x;
    const float* w;
    const float* scale;
    const float* shift;
    float* y;
    int hi, wi, ci, ho, wo, co, kw, stride, ph, pw, ldy, coff;
    int M, K;
};

template <int BM, int BN>
struct ICTile {
    static constexpr int WN = BN % 64 == 0 ? 2 : 1;  // 64, 128: 2 x 2 waves; 32, 96: four waves down the rows, each 32 x BN
    static constexpr int WM = 4 / WN;
    static constexpr int TM = BM / (32 * WM);
    static constexpr int TN = BN / (32 * WN);
    static_assert(TM >= 1 && TN >= 1 && TM * WM * 32 == BM && TN * WN * 32 == BN, "tile");
};

template <int BM, int BN, bool VEC>
__global__ __launch_bounds__(256) void infer_conv_k(ConvP p) {
    using T = ICTile<BM, BN>;
    constexpr int AC = BM / 32, BC = BN / 32;  // rows a thread stages per operand
    __shared__ __attribute__((aligned(16))) float As[BM * IC_LDR];
    __shared__ __attribute__((aligned(16))) float Bs[BN * IC_LDR];
    const float* __restrict__ X = p.x;
    const float* __restrict__ W = p.w;
    const int t = threadIdx.x, lane = t & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = t >> 6, wm = wave / T::WN, wn = wave % T::WN;
    const int kq = t & 7, r8 = t >> 3;  // the thread's 4-k chunk of the stage and its first row
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int M = p.M, K = p.K, ci = p.ci;

    // gathered rows: the (h0, w0) corner of the window and the offset of that corner (may point in front of the image: every
    // access is guarded by the bounds test of its tap)
    long long a_base[AC];
    int a_h0[AC], a_w0[AC];
    const int hw = p.ho * p.wo;
#pragma unroll
    for (int i = 0; i < AC; ++i) {
        const int m = m0 + r8 + 32 * i;
        const bool ok = m < M;
        const int mm = ok ? m : 0;
        const int img = mm / hw, rem = mm - img * hw;
        const int oh = rem / p.wo, ow = rem - oh * p.wo;
        const int h0 = oh * p.stride - p.ph, w0 = ow * p.stride - p.pw;
        a_base[i] = ((long long)(img * p.hi + h0) * p.wi + w0) * ci;
        a_h0[i] = ok ? h0 : -(1 << 20);  // a row past M: no tap brings it inside
        a_w0[i] = w0;
    }
    long long b_base[BC];
    bool b_ok[BC];
#pragma unroll
    for (int i = 0; i < BC; ++i) {
        const int n = n0 + r8 + 32 * i;
        b_ok[i] = n < p.co;
        b_base[i] = (long long)(b_ok[i] ? n : 0) * K;
    }

    f32x4 ra[AC], rb[BC];
    auto load_tile = [&](int kt) {
        const int k = kt * IC_BK + kq * 4;
        if constexpr (VEC) {  // K % 4 == 0: the chunk is whole or past the end, and lies inside one tap
            const bool kv = k < K;
            const int kk = kv ? k : 0;
            const int tap = kk / ci, c = kk - tap * ci;
            const int kh = tap / p.kw, kwi = tap - kh * p.kw;
            const int toff = (kh * p.wi + kwi) * ci + c;
#pragma unroll
            for (int i = 0; i < AC; ++i) {
                const int h = a_h0[i] + kh, w = a_w0[i] + kwi;
                const bool v = kv && (unsigned)h < (unsigned)p.hi && (unsigned)w < (unsigned)p.wi;
                ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (v) ra[i] = *reinterpret_cast<const f32x4*>(X + (a_base[i] + toff));
            }
#pragma unroll
            for (int i = 0; i < BC; ++i) {
                rb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (kv && b_ok[i]) rb[i] = *reinterpret_cast<const f32x4*>(W + (b_base[i] + kk));
            }
        } else {
#pragma unroll
            for (int i = 0; i < AC; ++i) ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < BC; ++i) rb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ke = k + e;
                if (ke >= K) continue;
                const int tap = ke / ci, c = ke - tap * ci;
                const int kh = tap / p.kw, kwi = tap - kh * p.kw;
                const int toff = (kh * p.wi + kwi) * ci + c;
#pragma unroll
                for (int i = 0; i < AC; ++i) {
                    const int h = a_h0[i] + kh, w = a_w0[i] + kwi;
                    if ((unsigned)h < (unsigned)p.hi && (unsigned)w < (unsigned)p.wi) ra[i][e] = X[a_base[i] + toff];
                }
#pragma unroll
                for (int i = 0; i < BC; ++i)
                    if (b_ok[i]) rb[i][e] = W[b_base[i] + ke];
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < AC; ++i) *reinterpret_cast<f32x4*>(As + (r8 + 32 * i) * IC_LDR + kq * 4) = ra[i];
#pragma unroll
        for (int i = 0; i < BC; ++i) *reinterpret_cast<f32x4*>(Bs + (r8 + 32 * i) * IC_LDR + kq * 4) = rb[i];
    };

    f32x16 acc[T::TM * T::TN];
#pragma unroll
    for (int i = 0; i < T::TM * T::TN; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    const int nk = (K + IC_BK - 1) / IC_BK;
    load_tile(0);
    store_tile();
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;  // (block-uniform)
        if (more) load_tile(kt + 1);
#pragma unroll
        for (int jj = 0; jj < IC_BK / 8; ++jj) {
            f32x4 a4[T::TM], b4[T::TN];
#pragma unroll
            for (int tn = 0; tn < T::TN; ++tn)
                b4[tn] = *reinterpret_cast<const f32x4*>(Bs + (wn * T::TN * 32 + tn * 32 + l31) * IC_LDR + half * (IC_BK / 2) + jj * 4);
#pragma unroll
            for (int tm = 0; tm < T::TM; ++tm)
                a4[tm] = *reinterpret_cast<const f32x4*>(As + (wm * T::TM * 32 + tm * 32 + l31) * IC_LDR + half * (IC_BK / 2) + jj * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < T::TN; ++tn)
                        acc[tm * T::TN + tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[tm][e], b4[tn][e], acc[tm * T::TN + tn], 0, 0, 0);
        }
        __syncthreads();
        if (more) {
            store_tile();
            __syncthreads();
        }
    }

    // accumulator register r of a lane: row (r & 3) + 8 (r >> 2) + 4 half of its 32x32 tile, column lane & 31
    float* __restrict__ Y = p.y;
#pragma unroll
    for (int tn = 0; tn < T::TN; ++tn) {
        const int n = n0 + wn * T::TN * 32 + tn * 32 + l31;
        if (n >= p.co) continue;
        const float sc = p.scale[n], sh = p.shift[n];
#pragma unroll
        for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * T::TM * 32 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (m < M) Y[(long long)m * p.ldy + p.coff + n] = fmaxf(fmaf(acc[tm * T::TN + tn][r], sc, sh), 0.f);
            }
    }
}

template <int BM, int BN>
void launch_conv(const ConvP& p, bool vec, hipStream_t st) {
    const dim3 grid((p.M + BM - 1) / BM, (p.co + BN - 1) / BN), block(256);
    if (vec) hipLaunchKernelGGL((infer_conv_k<BM, BN, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((infer_conv_k<BM, BN, false>), grid, block, 0, st, p);
}

// mode 0: max, stride 2, no padding; mode 1: average, stride 1, padding 1, / 9 always
__global__ __launch_bounds__(256) void infer_pool_k(const float* __restrict__ x, float* __restrict__ y, long long total, int h, int w,
                                                    int c, int ho, int wo, int mode, int ldy, int coff) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % c);
    const long long px = i / c;
    const int ow = (int)(px % wo);
    const long long q = px / wo;
    const int oh = (int)(q % ho), img = (int)(q / ho);
    const float* __restrict__ xi = x + (long long)img * h * w * c + ch;
    float out;
    if (mode == 0) {
        float m = -INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) m = fmaxf(m, xi[((long long)(2 * oh + a) * w + (2 * ow + b)) * c]);
        out = m;
    } else {
        double s = 0.0;
#pragma unroll
        for (int a = -1; a <= 1; ++a)
#pragma unroll
            for (int b = -1; b <= 1; ++b) {
                const int hh = oh + a, ww = ow + b;
                if ((unsigned)hh < (unsigned)h && (unsigned)ww < (unsigned)w) s += (double)xi[((long long)hh * w + ww) * c];
            }
        out = (float)(s / 9.0);
    }
    y[px * ldy + coff + ch] = out;
}

// the same, four channels per thread (c, ldy, coff multiples of 4, 16-byte aligned tensors)
__global__ __launch_bounds__(256) void infer_pool4_k(const float* __restrict__ x, float* __restrict__ y, long long total, int h, int w,
                                                     int c, int ho, int wo, int mode, int ldy, int coff) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int cq = c >> 2;
    const int ch = (int)(i % cq) * 4;
    const long long px = i / cq;
    const int ow = (int)(px % wo);
    const long long q = px / wo;
    const int oh = (int)(q % ho), img = (int)(q / ho);
    const float* __restrict__ xi = x + (long long)img * h * w * c + ch;
    f32x4 out;
    if (mode == 0) {
        f32x4 v[9];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) v[a * 3 + b] = *reinterpret_cast<const f32x4*>(xi + ((long long)(2 * oh + a) * w + (2 * ow + b)) * c);
        out = v[0];
#pragma unroll
        for (int k = 1; k < 9; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = fmaxf(out[j], v[k][j]);
    } else {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = -1; a <= 1; ++a)
#pragma unroll
            for (int b = -1; b <= 1; ++b) {
                const int hh = oh + a, ww = ow + b;
                if ((unsigned)hh < (unsigned)h && (unsigned)ww < (unsigned)w) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(xi + ((long long)hh * w + ww) * c);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s[j] += (double)v[j];
                }
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = (float)(s[j] / 9.0);
    }
    *reinterpret_cast<f32x4*>(y + px * ldy + coff + ch) = out;
}

__global__ __launch_bounds__(256) void infer_gmean_k(const float* __restrict__ x, float* __restrict__ y, int n, int hw, int c) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n * c) return;
    const int ch = (int)(i % c), img = (int)(i / c);
    const float* __restrict__ xi = x + (long long)img * hw * c + ch;
    double s = 0.0;
    for (int q = 0; q < hw; ++q) s += (double)xi[(long long)q * c];
    y[i] = (float)(s / (double)hw);
}

// Keys' cubic convolution kernel, a = -0.5 (the antialiased bicubic of F.interpolate / PIL)
__device__ __forceinline__ double keys(double x) {
    x = fabs(x);
    if (x < 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
    if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
    return 0.0;
}

// the triangle filter of the antialiased bilinear resize
__device__ __forceinline__ double triangle(double x) {
    x = fabs(x);
    return x < 1.0 ? 1.0 - x : 0.0;
}

// taps and normalised weights of output sample `o` (of the resized axis) over an input axis of `in` samples; scale = in / out <= 1.
// FILTER 0: Keys' cubic, support 2 (at most 5 taps); FILTER 1: the triangle, support 1 (at most 3 taps)
template <int FILTER>
__device__ __forceinline__ void taps_of(int o, double scale, int in, int& first, int& count, double (&wt)[5]) {
    constexpr double S = FILTER == 0 ? 2.0 : 1.0;
    constexpr int MAXT = FILTER == 0 ? 5 : 3;
    const double center = scale * (o + 0.5);
    int lo = (int)(center - S + 0.5);  // (truncation, as the int64 cast of the ATen routine)
    lo = lo < 0 ? 0 : lo;
    int hi = (int)(center + S + 0.5);
    hi = hi > in ? in : hi;
    first = lo;
    count = hi - lo;
    count = count > MAXT ? MAXT : count;
    double total = 0.0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        if constexpr (FILTER == 0) wt[j] = j < count ? keys((double)(j + lo) - center + 0.5) : 0.0;
        else wt[j] = j < count ? triangle((double)(j + lo) - center + 0.5) : 0.0;
        total += wt[j];
    }
    const double inv = total != 0.0 ? 1.0 / total : 0.0;
#pragma unroll
    for (int j = 0; j < 5; ++j) wt[j] *= inv;
}

template <int FILTER>
__global__ __launch_bounds__(256) void inception_prep_k(const float* __restrict__ x, float* __restrict__ y, int n, int h, int w, int rh,
                                                        int rw, int top, int left) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n * IC_OUT * IC_OUT) return;
    const int ox = (int)(i % IC_OUT);
    const long long q = i / IC_OUT;
    const int oy = (int)(q % IC_OUT), img = (int)(q / IC_OUT);
    int fy, cy, fx, cx;
    double wy[5], wx[5];
    taps_of<FILTER>(oy + top, (double)h / (double)rh, h, fy, cy, wy);
    taps_of<FILTER>(ox + left, (double)w / (double)rw, w, fx, cx, wx);
    const double mean[3] = {0.485, 0.456, 0.406}, stdv[3] = {0.229, 0.224, 0.225};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float* __restrict__ xc = x + ((long long)img * 3 + ch) * h * w;
        double s = 0.0;
        for (int a = 0; a < cy; ++a) {
            double r = 0.0;
            for (int b = 0; b < cx; ++b) {
                const float v = fminf(fmaxf(fmaf(xc[(long long)(fy + a) * w + fx + b], 0.5f, 0.5f), 0.f), 1.f);
                r += wx[b] * (double)v;
            }
            s += wy[a] * r;
        }
        y[i * 3 + ch] = (float)((s - mean[ch]) / stdv[ch]);
    }
}

inline bool ic_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
constexpr long long IC_LIMIT = 1LL << 31;

}  // namespace

extern "C" int movae_infer_conv2d(const float* x, const float* w, const float* scale, const float* shift, float* y, int n, int h, int wd,
                                  int ci, int co, int kh, int kw, int stride, int pad_h, int pad_w, int ldy, int coff,
                                  movae_stream_t stream) {
    MOVAE_CHECK_ARG(x && w && scale && shift && y, "movae_infer_conv2d: null pointer");
    MOVAE_CHECK_ARG(n > 0 && h > 0 && wd > 0 && ci > 0 && co > 0, "movae_infer_conv2d: empty shape n %d h %d w %d ci %d co %d", n, h, wd, ci,
                    co);
    MOVAE_CHECK_ARG(kh >= 1 && kh <= 7 && kw >= 1 && kw <= 7 && stride >= 1, "movae_infer_conv2d: kernel %d x %d stride %d (sides 1..7)", kh,
                    kw, stride);
    MOVAE_CHECK_ARG(pad_h >= 0 && pad_h < kh && pad_w >= 0 && pad_w < kw, "movae_infer_conv2d: padding (%d, %d) must stay below the kernel %d x %d",
                    pad_h, pad_w, kh, kw);
    MOVAE_CHECK_ARG(h + 2 * pad_h >= kh && wd + 2 * pad_w >= kw, "movae_infer_conv2d: a %d x %d kernel does not fit %d x %d with padding (%d, %d)",
                    kh, kw, h, wd, pad_h, pad_w);
    const int ho = (h + 2 * pad_h - kh) / stride + 1, wo = (wd + 2 * pad_w - kw) / stride + 1;
    MOVAE_CHECK_ARG(coff >= 0 && ldy >= coff + co, "movae_infer_conv2d: channels %d .. %d do not fit an output row of %d", coff, coff + co, ldy);
    const long long M = (long long)n * ho * wo, K = (long long)kh * kw * ci;
    MOVAE_CHECK_ARG(M < IC_LIMIT && (long long)n * h * wd * ci < IC_LIMIT && M * ldy < IC_LIMIT * 4 && K * co < IC_LIMIT,
                    "movae_infer_conv2d: the shape is too large (n %d, %d x %d x %d -> %d x %d x %d)", n, h, wd, ci, ho, wo, ldy);
    ConvP p{x, w, scale, shift, y, h, wd, ci, ho, wo, co, kw, stride, pad_h, pad_w, ldy, coff, (int)M, (int)K};
    const bool vec = ci % 4 == 0 && ic_aligned16(x) && ic_aligned16(w);
    // the column tile that pads co least, tried in the order of their measured efficiency (2 x 2 waves of 64 x 64 / 64 x 32 first;
    // the four-waves-down tiles 128 x 96 and 128 x 32 only where they pad strictly less: co = 96 takes one 96-column tile instead
    // of three 32-column ones, co = 192 stays with three 64-column tiles); short row counts take the 64-row tile to fill the machine
    int bn = 128;
    long long best = ((co + 127) / 128) * 128LL;
    for (int cand : {64, 96, 32}) {
        const long long padded = ((co + cand - 1) / cand) * (long long)cand;
        if (padded < best) best = padded, bn = cand;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (bn == 128) launch_conv<128, 128>(p, vec, st);
    else if (bn == 96) launch_conv<128, 96>(p, vec, st);
    else if (bn == 32) launch_conv<128, 32>(p, vec, st);
    else if (((M + 127) / 128) * ((co + 63) / 64) < 256) launch_conv<64, 64>(p, vec, st);
    else launch_conv<128, 64>(p, vec, st);
    MOVAE_CHECK_LAUNCH("infer_conv_k");
    return MOVAE_OK;
}

extern "C" int movae_infer_pool3x3(const float* x, float* y, int n, int h, int w, int c, int mode, int ldy, int coff, movae_stream_t stream) {
    MOVAE_CHECK_ARG(x && y, "movae_infer_pool3x3: null pointer");
    MOVAE_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0, "movae_infer_pool3x3: empty shape %d x %d x %d x %d", n, h, w, c);
    MOVAE_CHECK_ARG(mode == 0 || mode == 1, "movae_infer_pool3x3: mode %d (0 max / stride 2, 1 average / stride 1)", mode);
    MOVAE_CHECK_ARG(mode == 1 || (h >= 3 && w >= 3), "movae_infer_pool3x3: the unpadded 3x3 window does not fit %d x %d", h, w);
    MOVAE_CHECK_ARG(coff >= 0 && ldy >= coff + c, "movae_infer_pool3x3: channels %d .. %d do not fit an output row of %d", coff, coff + c, ldy);
    const int ho = mode == 0 ? (h - 3) / 2 + 1 : h, wo = mode == 0 ? (w - 3) / 2 + 1 : w;
    const long long total = (long long)n * ho * wo * c;
    MOVAE_CHECK_ARG((long long)n * h * w * c < IC_LIMIT && (long long)n * ho * wo * ldy < IC_LIMIT * 4, "movae_infer_pool3x3: the shape is too large");
    if (c % 4 == 0 && ldy % 4 == 0 && coff % 4 == 0 && ic_aligned16(x) && ic_aligned16(y)) {
        const long long quads = total / 4;
        hipLaunchKernelGGL(infer_pool4_k, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, quads, h,
                           w, c, ho, wo, mode, ldy, coff);
    } else {
        hipLaunchKernelGGL(infer_pool_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, total, h, w,
                           c, ho, wo, mode, ldy, coff);
    }
    MOVAE_CHECK_LAUNCH("infer_pool_k");
    return MOVAE_OK;
}

extern "C" int movae_infer_global_mean(const float* x, float* y, int n, int hw, int c, movae_stream_t stream) {
    MOVAE_CHECK_ARG(x && y, "movae_infer_global_mean: null pointer");
    MOVAE_CHECK_ARG(n > 0 && hw > 0 && c > 0, "movae_infer_global_mean: empty shape %d x %d x %d", n, hw, c);
    MOVAE_CHECK_ARG((long long)n * hw * c < IC_LIMIT, "movae_infer_global_mean: the shape is too large");
    const long long total = (long long)n * c;
    hipLaunchKernelGGL(infer_gmean_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, n, hw, c);
    MOVAE_CHECK_LAUNCH("infer_gmean_k");
    return MOVAE_OK;
}

extern "C" int movae_inception_prep_filter(const float* x, float* y, int n, int h, int w, int filter, movae_stream_t stream) {
    MOVAE_CHECK_ARG(x && y, "movae_inception_prep: null pointer");
    MOVAE_CHECK_ARG(n > 0 && h > 0 && w > 0, "movae_inception_prep: empty shape %d x 3 x %d x %d", n, h, w);
    MOVAE_CHECK_ARG(h <= IC_OUT && w <= IC_OUT, "movae_inception_prep: %d x %d has a side above %d (reducing needs a true antialiasing filter)", h,
                    w, IC_OUT);
    MOVAE_CHECK_ARG(filter == MOVAE_RESIZE_BICUBIC || filter == MOVAE_RESIZE_BILINEAR, "movae_inception_prep: filter %d (0 bicubic, 1 bilinear)",
                    filter);
    MOVAE_CHECK_ARG((long long)n * IC_OUT * IC_OUT * 3 < IC_LIMIT * 4, "movae_inception_prep: n %d is too large", n);
    // TF.resize(299): the shorter side to 299, the other to int(299 * long / short); TF.center_crop: round-half-even offsets
    int rh, rw;
    if (h <= w) rh = IC_OUT, rw = (int)((long long)IC_OUT * w / h);
    else rw = IC_OUT, rh = (int)((long long)IC_OUT * h / w);
    const int top = (int)nearbyint((rh - IC_OUT) / 2.0), left = (int)nearbyint((rw - IC_OUT) / 2.0);
    const long long total = (long long)n * IC_OUT * IC_OUT;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (filter == MOVAE_RESIZE_BICUBIC) hipLaunchKernelGGL(inception_prep_k<0>, grid, block, 0, st, x, y, n, h, w, rh, rw, top, left);
    else hipLaunchKernelGGL(inception_prep_k<1>, grid, block, 0, st, x, y, n, h, w, rh, rw, top, left);
    MOVAE_CHECK_LAUNCH("inception_prep_k");
    return MOVAE_OK;
}

extern "C" int movae_inception_prep(const float* x, float* y, int n, int h, int w, movae_stream_t stream) {
    return movae_inception_prep_filter(x, y, n, h, w, MOVAE_RESIZE_BICUBIC, stream);
}
