// Reconstruction metrics of the final evaluation (reference main.py:335-373 over utils/metrics.py:14-80 ssim, :108-154 ssnr,
// :157-203 psnr): SSIM with the 11x11 (window_size) Gaussian window, MSE / PSNR and SSNR of a chunk of (real, recon) image pairs.
//
// Three launches per chunk, no host read:
//   metric_min_k        per-block minima of each operand (metrics.py:47-55 decides the normalisation on chunk.min() < 0)
//   metric_ssim_k<R>    one workgroup per (32x32 output tile, channel, image): every block folds the (few) per-block minima
//                       into the two normalisation flags itself, then both images' halo tile is normalised into LDS, the
//                       horizontal pass of the five fields x, y, x^2, y^2, xy goes to LDS, the vertical pass and the SSIM map
//                       stay in registers; per-block partials of sum ssim, sum (x-y)^2, sum x, sum x^2 in fp64
//   metric_finalize_k   one block folds the partials in a fixed order: per-image SSIM / MSE / SSNR and the chunk's ssim / psnr
// No float atomics and no in-launch hand-offs (each kernel boundary orders the next one's reads): every sum has a fixed order, so
// results are bit-identical from run to run.  (A last-block fold through a workspace counter measured slower
// here: with hundreds of blocks the agent-scope release of every block cost more than the finalize launch it saved.)
#include "common.h"

#include <math.h>

namespace {

constexpr int MT = 32;        // output tile side
constexpr int MT_THREADS = 256;
constexpr int MIN_BLOCKS = 512;  // cap of the min pass's grid (every SSIM block folds its partials)
constexpr int MIN_UNROLL = 4;    // float4s per thread and operand in flight at once

struct Strides {
    long long n, c, h, w;
};

struct Window {
    float g[16];
};

__device__ __forceinline__ float norm_px(float v, int shift) {
    if (shift) v = (v + 1.f) * 0.5f;  // (img + 1) / 2: division by two is exact either way
    return fminf(fmaxf(v, 0.f), 1.f);
}

// ---- per-block minima of both operands -----------------------------------------------------------------------------------
// dense != 0: the operand's strides are a permutation of a packed layout, so its elements are the `total` floats from p on
// (the min does not care about their order); vec4 != 0 additionally: p is 16-byte aligned and total % 4 == 0.  The pass is
// latency-bound: in the common case (both operands dense, vec4) a thread has MIN_UNROLL float4s of each in flight at once.
__device__ __forceinline__ float elem(const float* __restrict__ p, Strides s, int C, int H, int W, long long i, int dense) {
    if (dense) return p[i];
    long long r = i;
    const int w = (int)(r % W);
    r /= W;
    const int h = (int)(r % H);
    r /= H;
    const int c = (int)(r % C);
    const long long n = r / C;
    return p[n * s.n + c * s.c + h * s.h + w * s.w];
}

__device__ __forceinline__ float min4(f32x4 v) { return fminf(fminf(v[0], v[1]), fminf(v[2], v[3])); }

__global__ __launch_bounds__(MT_THREADS) void metric_min_k(const float* __restrict__ a, Strides sa, int a_dense, int a_vec4,
                                                           const float* __restrict__ b, Strides sb, int b_dense, int b_vec4,
                                                           int C, int H, int W, long long total, float* __restrict__ part) {
    __shared__ float sh[2][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float ma = INFINITY, mb = INFINITY;
    if (a_vec4 && b_vec4) {
        const long long n4 = total >> 2;
        const f32x4* a4 = reinterpret_cast<const f32x4*>(a);
        const f32x4* b4 = reinterpret_cast<const f32x4*>(b);
        const f32x4 inf4 = {INFINITY, INFINITY, INFINITY, INFINITY};
        for (long long i0 = t0; i0 < n4; i0 += MIN_UNROLL * stride) {
            f32x4 va[MIN_UNROLL], vb[MIN_UNROLL];
#pragma unroll
            for (int u = 0; u < MIN_UNROLL; ++u) {
                const long long i = i0 + u * stride;
                va[u] = i < n4 ? a4[i] : inf4;
                vb[u] = i < n4 ? b4[i] : inf4;
            }
#pragma unroll
            for (int u = 0; u < MIN_UNROLL; ++u) {
                ma = fminf(ma, min4(va[u]));
                mb = fminf(mb, min4(vb[u]));
            }
        }
    } else {
        // per operand: float4s where it allows them (4 elements per index), else single elements
        const long long na = a_vec4 ? total >> 2 : total, nb = b_vec4 ? total >> 2 : total;
        for (long long i = t0; i < (na > nb ? na : nb); i += stride) {
            if (i < na) ma = fminf(ma, a_vec4 ? min4(reinterpret_cast<const f32x4*>(a)[i]) : elem(a, sa, C, H, W, i, a_dense));
            if (i < nb) mb = fminf(mb, b_vec4 ? min4(reinterpret_cast<const f32x4*>(b)[i]) : elem(b, sb, C, H, W, i, b_dense));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ma = fminf(ma, __shfl_xor(ma, o, 64));
        mb = fminf(mb, __shfl_xor(mb, o, 64));
    }
    if (lane == 0) {
        sh[0][wave] = ma;
        sh[1][wave] = mb;
    }
    __syncthreads();
    if (t < 2) part[t * gridDim.x + blockIdx.x] = fminf(fminf(sh[t][0], sh[t][1]), fminf(sh[t][2], sh[t][3]));
}

// ---- the fused SSIM / MSE / signal-statistics pass ---------------------------------------------------------------------
// LDS (dynamic, 16-byte aligned base; every carve offset a multiple of 16 bytes):
//   red   [4 waves][4]      doubles, the block's partial sums
//   xs/ys [HALO][XP]        normalised halo tiles (zero outside the image: F.conv2d's zero padding of the normalised image)
//   h     [5][HALO][HP]     horizontal pass of x, y, x^2, y^2, xy over every halo row, for the tile's 32 output columns
// XP is odd and HP = 33: the column reads of the vertical pass and the row-shifted reads of the horizontal pass spread
// over the banks instead of landing on one (a 32-float row stride would put the two row groups of a wave on one bank).
template <int R>
struct SsimGeom {
    static constexpr int HALO = MT + 2 * R;
    static constexpr int XP = HALO | 1;
    static constexpr int HP = MT + 1;
    static constexpr int RED_BYTES = 4 * 4 * 8;
    static constexpr int XS_FLOATS = (HALO * XP + 3) & ~3;
    static constexpr int H_FLOATS = (HALO * HP + 3) & ~3;
    static constexpr int BYTES = RED_BYTES + 2 * XS_FLOATS * 4 + 5 * H_FLOATS * 4;
};

// Stages one operand's halo tile in two steps, so that the loads of both operands are in flight together (the staging is
// latency-bound: a loop of load -> store iterations would wait out one memory latency per iteration).
// vec4: w-stride 1, every row start 16-byte aligned and W % 4 == 0 -- the row segment is read as aligned float4s, each of which
// lies wholly inside or wholly outside [0, W); otherwise element loads through the strides (the decoder's NHWC buffer seen as
// NCHW has a w-stride of C).
template <int R>
struct TileLoad {
    using G = SsimGeom<R>;
    static constexpr int RA = (R + 3) & ~3;        // halo rounded up to whole float4s
    static constexpr int NV = (MT + 2 * RA) / 4;   // float4s per halo row
    static constexpr int NQ = (G::HALO * NV + MT_THREADS - 1) / MT_THREADS;
    static constexpr int NS = (G::HALO * G::HALO + MT_THREADS - 1) / MT_THREADS;
    f32x4 q[NQ];
    float e[NS];

    __device__ __forceinline__ void load(const float* __restrict__ src, Strides s, int vec4, int H, int W, int y0, int x0) {
        const int t = threadIdx.x;
        if (vec4) {
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const int i = t + k * MT_THREADS;
                const int r = i / NV, j = i - r * NV;
                const int gy = y0 - R + r, gx = x0 - RA + 4 * j;
                q[k] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (i < G::HALO * NV && gy >= 0 && gy < H && gx >= 0 && gx < W) q[k] = *reinterpret_cast<const f32x4*>(src + gy * s.h + gx);
            }
        } else {
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int i = t + k * MT_THREADS;
                const int r = i / G::HALO, cc = i - r * G::HALO;
                const int gy = y0 - R + r, gx = x0 - R + cc;
                e[k] = 0.f;
                if (i < G::HALO * G::HALO && gy >= 0 && gy < H && gx >= 0 && gx < W) e[k] = src[gy * s.h + gx * s.w];
            }
        }
    }

    // zero outside the image: F.conv2d pads the NORMALISED image with zeros (norm_px(0) would be 0.5 for a [-1, 1] operand)
    __device__ __forceinline__ void store(float* __restrict__ dst, int vec4, int shift, int H, int W, int y0, int x0) const {
        const int t = threadIdx.x;
        if (vec4) {
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const int i = t + k * MT_THREADS;
                if (i >= G::HALO * NV) continue;
                const int r = i / NV, j = i - r * NV;
                const int gy = y0 - R + r, gx = x0 - RA + 4 * j;
                const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int cc = gx + u - (x0 - R);
                    if (cc >= 0 && cc < G::HALO) dst[r * G::XP + cc] = in ? norm_px(q[k][u], shift) : 0.f;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int i = t + k * MT_THREADS;
                if (i >= G::HALO * G::HALO) continue;
                const int r = i / G::HALO, cc = i - r * G::HALO;
                const int gy = y0 - R + r, gx = x0 - R + cc;
                dst[r * G::XP + cc] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? norm_px(e[k], shift) : 0.f;
            }
        }
    }
};

// ---- finalize: one block, fixed order -----------------------------------------------------------------------------------
// out[0] ssim (mean of the map over n c h w), out[1] psnr, out[2] ssnr (means over the images), then per image:
// out[3 + i] ssim, out[3 + n + i] mse, out[3 + 2 n + i] ssnr (dB)
__global__ __launch_bounds__(MT_THREADS) void metric_finalize_k(const double* __restrict__ part, int n, int parts_per_image,
                                                                long long m, float max_val, float* __restrict__ out) {
    __shared__ double sh[4];
    const int t = threadIdx.x;
    double t_ssim = 0.0, t_psnr = 0.0, t_ssnr = 0.0;
    const double md = (double)m;
    const double peak = 20.0 * log10((double)max_val);
    for (int i = t; i < n; i += MT_THREADS) {
        double s_ssim = 0.0, s_d2 = 0.0, s_x = 0.0, s_x2 = 0.0;
        const double* p = part + (long long)i * parts_per_image * 4;
        for (int q = 0; q < parts_per_image; ++q) {
            s_ssim += p[4 * q + 0];
            s_d2 += p[4 * q + 1];
            s_x += p[4 * q + 2];
            s_x2 += p[4 * q + 3];
        }
        const double mse = s_d2 / md;
        const double var = (s_x2 - s_x * (s_x / md)) / (md - 1.0);  // torch.var: unbiased
        const double mse_c = fmax(mse, 1e-10), var_c = fmax(var, 1e-10);
        const double psnr = peak - 10.0 * log10(mse_c);
        const double ssnr = 10.0 * log10(var_c / mse_c);
        out[3 + i] = (float)(s_ssim / md);
        out[3 + n + i] = (float)mse;
        out[3 + 2 * n + i] = (float)ssnr;
        t_ssim += s_ssim;
        t_psnr += psnr;
        t_ssnr += ssnr;
    }
    const double a = block_sum_256(t_ssim, sh);
    const double b = block_sum_256(t_psnr, sh);
    const double c = block_sum_256(t_ssnr, sh);
    if (t == 0) {
        out[0] = (float)(a / (md * n));
        out[1] = (float)(b / n);
        out[2] = (float)(c / n);
    }
}

template <int R>
__global__ __launch_bounds__(MT_THREADS) void metric_ssim_k(const float* __restrict__ a, Strides sa, int a_vec4,
                                                            const float* __restrict__ b, Strides sb, int b_vec4, int H, int W,
                                                            int tiles_x, Window win, const float* __restrict__ minpart,
                                                            int nmin, double* __restrict__ part) {
    using G = SsimGeom<R>;
    constexpr int K = 2 * R + 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* red = reinterpret_cast<double*>(smem);
    float* xs = reinterpret_cast<float*>(smem + G::RED_BYTES);
    float* ys = xs + G::XS_FLOATS;
    float* hf = ys + G::XS_FLOATS;  // [5][HALO][HP]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tile = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * MT, x0 = tx * MT;
    float g[K];
#pragma unroll
    for (int k = 0; k < K; ++k) g[k] = win.g[k];

    {
        TileLoad<R> la, lb;
        la.load(a + n * sa.n + c * sa.c, sa, a_vec4, H, W, y0, x0);
        lb.load(b + n * sb.n + c * sb.c, sb, b_vec4, H, W, y0, x0);
        // the normalisation flags: min over the min pass's per-block partials (while the tile loads are in flight)
        float ma = INFINITY, mb = INFINITY;
        for (int i = t; i < nmin; i += MT_THREADS) {
            ma = fminf(ma, minpart[i]);
            mb = fminf(mb, minpart[nmin + i]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            ma = fminf(ma, __shfl_xor(ma, o, 64));
            mb = fminf(mb, __shfl_xor(mb, o, 64));
        }
        float* fl = reinterpret_cast<float*>(red);
        if (lane == 0) {
            fl[wave] = ma;
            fl[4 + wave] = mb;
        }
        __syncthreads();
        const int fa = fminf(fminf(fl[0], fl[1]), fminf(fl[2], fl[3])) < 0.f;
        const int fb = fminf(fminf(fl[4], fl[5]), fminf(fl[6], fl[7])) < 0.f;
        la.store(xs, a_vec4, fa, H, W, y0, x0);
        lb.store(ys, b_vec4, fb, H, W, y0, x0);
    }
    __syncthreads();

    // horizontal pass: every halo row, the tile's 32 output columns
    for (int i = t; i < G::HALO * MT; i += MT_THREADS) {
        const int r = i >> 5, col = i & 31;
        const float* xr = xs + r * G::XP + col;
        const float* yr = ys + r * G::XP + col;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float xv = xr[k], yv = yr[k];
            s0 = fmaf(g[k], xv, s0);
            s1 = fmaf(g[k], yv, s1);
            s2 = fmaf(g[k], xv * xv, s2);
            s3 = fmaf(g[k], yv * yv, s3);
            s4 = fmaf(g[k], xv * yv, s4);
        }
        const int o = r * G::HP + col;
        hf[0 * G::HALO * G::HP + o] = s0;
        hf[1 * G::HALO * G::HP + o] = s1;
        hf[2 * G::HALO * G::HP + o] = s2;
        hf[3 * G::HALO * G::HP + o] = s3;
        hf[4 * G::HALO * G::HP + o] = s4;
    }
    __syncthreads();

    // vertical pass in registers: thread (col, rg) owns output rows 4 rg .. 4 rg + 3 of column col
    const int col = t & 31, rg = t >> 5;
    float acc[5][4];
#pragma unroll
    for (int f = 0; f < 5; ++f) {
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[f][o] = 0.f;
        const float* hc = hf + f * G::HALO * G::HP + (4 * rg) * G::HP + col;
#pragma unroll
        for (int j = 0; j < K + 3; ++j) {
            const float v = hc[j * G::HP];
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if (j - o >= 0 && j - o < K) acc[f][o] = fmaf(g[j - o], v, acc[f][o]);
        }
    }
    const float C1 = 1e-4f, C2 = 9e-4f;  // the reference's 0.01 ** 2, 0.03 ** 2 as they meet an fp32 tensor
    double s_ssim = 0.0, s_d2 = 0.0, s_x = 0.0, s_x2 = 0.0;
    const int gx = x0 + col;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int ly = 4 * rg + o, gy = y0 + ly;
        if (gy < H && gx < W) {
            const float mu1 = acc[0][o], mu2 = acc[1][o];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
            const float s1 = acc[2][o] - mu1_sq, s2 = acc[3][o] - mu2_sq, s12 = acc[4][o] - mu1_mu2;
            const float map = ((2.f * mu1_mu2 + C1) * (2.f * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
            const float xv = xs[(ly + R) * G::XP + col + R], yv = ys[(ly + R) * G::XP + col + R];
            const double d = (double)xv - (double)yv;
            s_ssim += (double)map;
            s_d2 += d * d;
            s_x += (double)xv;
            s_x2 += (double)xv * (double)xv;
        }
    }
    s_ssim = wave_sum(s_ssim);
    s_d2 = wave_sum(s_d2);
    s_x = wave_sum(s_x);
    s_x2 = wave_sum(s_x2);
    if (lane == 0) {
        red[wave * 4 + 0] = s_ssim;
        red[wave * 4 + 1] = s_d2;
        red[wave * 4 + 2] = s_x;
        red[wave * 4 + 3] = s_x2;
    }
    __syncthreads();
    if (t < 4) {
        const long long blk = ((long long)n * gridDim.y + c) * gridDim.x + tile;
        part[blk * 4 + t] = (red[t] + red[4 + t]) + (red[8 + t] + red[12 + t]);
    }
}

// the reference's window: the 1-D Gaussian (sigma 1.5) drawn in float64, stored as float32 and normalised in float32
Window make_window(int ws) {
    Window w{};
    float sum = 0.f;
    for (int i = 0; i < ws; ++i) {
        const double d = (double)(i - ws / 2);
        w.g[i] = (float)exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += w.g[i];
    }
    for (int i = 0; i < ws; ++i) w.g[i] /= sum;
    return w;
}

bool is_dense(Strides s, int n, int c, int h, int w) {
    long long st[4] = {s.n, s.c, s.h, s.w};
    long long sz[4] = {n, c, h, w};
    // order the dimensions by stride (sizes of 1 may carry any stride: give them none)
    for (int i = 0; i < 4; ++i)
        if (sz[i] == 1) st[i] = 0;
    int idx[4] = {0, 1, 2, 3};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (st[idx[j]] < st[idx[i]]) {
                const int tmp = idx[i];
                idx[i] = idx[j];
                idx[j] = tmp;
            }
    long long expect = 1;
    for (int i = 0; i < 4; ++i) {
        const int d = idx[i];
        if (sz[d] == 1) continue;
        if (st[d] != expect) return false;
        expect *= sz[d];
    }
    return true;
}

struct Plan {
    int tiles_x, tiles;
    long long total;
    int min_blocks;
    size_t off_min, off_part, bytes;
};

Plan plan_of(int n, int c, int h, int w) {
    Plan p;
    p.tiles_x = (w + MT - 1) / MT;
    p.tiles = p.tiles_x * ((h + MT - 1) / MT);
    p.total = (long long)n * c * h * w;
    const long long want = (p.total / 4 + MT_THREADS * MIN_UNROLL - 1) / (MT_THREADS * MIN_UNROLL);
    p.min_blocks = (int)(want < 1 ? 1 : (want > MIN_BLOCKS ? MIN_BLOCKS : want));
    p.off_min = MOVAE_WS_HEADER_BYTES;  // (the header is not used: no hand-off counter)
    p.off_part = p.off_min + (((size_t)2 * MIN_BLOCKS * sizeof(float) + 255) & ~(size_t)255);
    p.bytes = p.off_part + (size_t)n * c * p.tiles * 4 * sizeof(double);
    return p;
}

template <int R>
int launch_ssim(const float* a, Strides sa, int a_vec4, const float* b, Strides sb, int b_vec4, int n, int c, int h, int w,
                const Plan& p, const Window& win, const float* minpart, double* part, hipStream_t st) {
    const size_t lds = SsimGeom<R>::BYTES;
    hipLaunchKernelGGL(metric_ssim_k<R>, dim3(p.tiles, c, n), dim3(MT_THREADS), lds, st, a, sa, a_vec4, b, sb, b_vec4, h, w,
                       p.tiles_x, win, minpart, p.min_blocks, part);
    MOVAE_CHECK_LAUNCH("metric_ssim_k");
    return MOVAE_OK;
}

}  // namespace

extern "C" size_t movae_recon_metrics_ws_bytes(int n, int c, int h, int w) {
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return 0;
    return plan_of(n, c, h, w).bytes;
}

extern "C" int movae_recon_metrics(const float* real, long long rs_n, long long rs_c, long long rs_h, long long rs_w,
                                   const float* recon, long long ps_n, long long ps_c, long long ps_h, long long ps_w, int n, int c,
                                   int h, int w, int window_size, float max_val, float* out, void* ws, size_t ws_bytes,
                                   movae_stream_t stream) {
    MOVAE_CHECK_ARG(real && recon && out && ws, "movae_recon_metrics: null pointer");
    MOVAE_CHECK_ARG(n > 0 && c > 0 && h > 0 && w > 0, "movae_recon_metrics: empty shape %d x %d x %d x %d", n, c, h, w);
    MOVAE_CHECK_ARG(n <= 65535 && c <= 65535, "movae_recon_metrics: n %d / c %d above the grid limit", n, c);
    MOVAE_CHECK_ARG(window_size >= 3 && window_size <= 15 && (window_size & 1), "movae_recon_metrics: window_size %d (odd, 3..15)",
                    window_size);
    const Plan p = plan_of(n, c, h, w);
    MOVAE_CHECK_ARG(ws_bytes >= p.bytes, "movae_recon_metrics: workspace %zu bytes < %zu", ws_bytes, p.bytes);
    const Strides sa{rs_n, rs_c, rs_h, rs_w}, sb{ps_n, ps_c, ps_h, ps_w};
    char* base = static_cast<char*>(ws);
    float* minpart = reinterpret_cast<float*>(base + p.off_min);
    double* part = reinterpret_cast<double*>(base + p.off_part);
    hipStream_t st = static_cast<hipStream_t>(stream);

    auto aligned16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const int a_dense = is_dense(sa, n, c, h, w), b_dense = is_dense(sb, n, c, h, w);
    const int a_min4 = a_dense && aligned16(real) && (p.total & 3) == 0;
    const int b_min4 = b_dense && aligned16(recon) && (p.total & 3) == 0;
    // the SSIM pass reads float4s along w: w-stride 1, image / channel / row starts on 16-byte boundaries
    const int a_vec4 = rs_w == 1 && (w & 3) == 0 && (rs_h & 3) == 0 && (rs_c & 3) == 0 && (rs_n & 3) == 0 && aligned16(real);
    const int b_vec4 = ps_w == 1 && (w & 3) == 0 && (ps_h & 3) == 0 && (ps_c & 3) == 0 && (ps_n & 3) == 0 && aligned16(recon);

    hipLaunchKernelGGL(metric_min_k, dim3(p.min_blocks), dim3(MT_THREADS), 0, st, real, sa, a_dense, a_min4, recon, sb, b_dense,
                       b_min4, c, h, w, p.total, minpart);
    MOVAE_CHECK_LAUNCH("metric_min_k");
    const Window win = make_window(window_size);
    int rc = MOVAE_OK;
    switch (window_size / 2) {
        case 1: rc = launch_ssim<1>(real, sa, a_vec4, recon, sb, b_vec4, n, c, h, w, p, win, minpart, part, st); break;
        case 2: rc = launch_ssim<2>(real, sa, a_vec4, recon, sb, b_vec4, n, c, h, w, p, win, minpart, part, st); break;
        case 3: rc = launch_ssim<3>(real, sa, a_vec4, recon, sb, b_vec4, n, c, h, w, p, win, minpart, part, st); break;
        case 4: rc = launch_ssim<4>(real, sa, a_vec4, recon, sb, b_vec4, n, c, h, w, p, win, minpart, part, st); break;
        case 5: rc = launch_ssim<5>(real, sa, a_vec4, recon, sb, b_vec4, n, c, h, w, p, win, minpart, part, st); break;
        case 6: rc = launch_ssim<6>(real, sa, a_vec4, recon, sb, b_vec4, n, c, h, w, p, win, minpart, part, st); break;
        default: rc = launch_ssim<7>(real, sa, a_vec4, recon, sb, b_vec4, n, c, h, w, p, win, minpart, part, st); break;
    }
    if (rc != MOVAE_OK) return rc;
    hipLaunchKernelGGL(metric_finalize_k, dim3(1), dim3(MT_THREADS), 0, st, part, n, c * p.tiles, (long long)c * h * w, max_val, out);
    MOVAE_CHECK_LAUNCH("metric_finalize_k");
    return MOVAE_OK;
}
