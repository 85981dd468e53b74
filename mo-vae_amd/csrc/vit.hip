// The row operators of the ViT Sphere Encoder (reference models/sphere_encoder_vit.py): LayerNorm / RMSNorm over the last dimension of
// a row-major [rows, D] tensor (:34-50 RMSNorm, nn.LayerNorm in TransformerBlock :175-177), the exact (erf) GELU on a conv's output
// plus its bias (:179-185, :199-209), Unpatchify + tanh (:125-140, :388) and the broadcast add of a positional table (:53-68).
// All fp32; every reduction runs in a fixed order and nothing uses float atomics, so reruns are bit-identical.
//
// Row norm.  LPR lanes own a row (64: one wave per row; 8 for D <= 32, so that a 256-thread block covers 32 rows instead of 4); each
// lane strides over the row, the partial sums meet in an xor butterfly of width LPR.  Mean first, then the centred second moment (the
// biased variance as nn.LayerNorm forms it), re-reading the row from cache.  The weight / bias gradients are column sums over the
// rows: stage one leaves one partial row per block of RB rows in the workspace, stage two folds the partials in order.
#include "common.h"

namespace {

constexpr int MODE_LN = 0, MODE_RMS = 1;

template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// out[row][d] = xhat * w[d] + b[d] + pos[row % period][d];  xhat = (x - mean) * rstd (LayerNorm) or x * rstd (RMSNorm)
template <int LPR, int MODE>
__global__ __launch_bounds__(256) void rownorm_fwd_k(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                     const float* __restrict__ pos, float* __restrict__ out, float* __restrict__ mean_out,
                                                     float* __restrict__ rstd_out, long rows, int D, int period, float eps) {
    constexpr int RPB = 256 / LPR;
    const int sub = threadIdx.x % LPR;
    const long row = (long)blockIdx.x * RPB + threadIdx.x / LPR;
    const bool live = row < rows;  // (dead rows keep their lanes in the butterflies)
    const float* xr = x + (live ? row : 0) * D;
    const float inv_d = 1.f / (float)D;
    float mean = 0.f;
    if (MODE == MODE_LN) {
        float s = 0.f;
        if (live)
            for (int d = sub; d < D; d += LPR) s += xr[d];
        mean = group_sum<LPR>(s) * inv_d;
    }
    float s2 = 0.f;
    if (live)
        for (int d = sub; d < D; d += LPR) {
            const float c = xr[d] - mean;
            s2 += c * c;
        }
    const float rstd = 1.f / sqrtf(group_sum<LPR>(s2) * inv_d + eps);
    if (!live) return;
    const float* pr = pos ? pos + (row % period) * D : nullptr;
    float* orow = out + row * D;
    for (int d = sub; d < D; d += LPR) {
        float y = (xr[d] - mean) * rstd;
        if (w) y *= w[d];
        if (b) y += b[d];
        if (pr) y += pr[d];
        orow[d] = y;
    }
    if (sub == 0) {
        rstd_out[row] = rstd;
        if (MODE == MODE_LN) mean_out[row] = mean;
    }
}

// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)) with g = dy * w  (RMSNorm: without the mean(g) term)
template <int LPR, int MODE>
__global__ __launch_bounds__(256) void rownorm_bwd_dx_k(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                        float* __restrict__ dx, long rows, int D) {
    constexpr int RPB = 256 / LPR;
    const int sub = threadIdx.x % LPR;
    const long row = (long)blockIdx.x * RPB + threadIdx.x / LPR;
    const bool live = row < rows;
    const long r = live ? row : 0;
    const float *xr = x + r * D, *gr = dy + r * D;
    const float mean = MODE == MODE_LN ? mean_in[r] : 0.f, rstd = rstd_in[r];
    float sg = 0.f, sgx = 0.f;
    if (live)
        for (int d = sub; d < D; d += LPR) {
            const float g = w ? gr[d] * w[d] : gr[d];
            sg += g;
            sgx += g * ((xr[d] - mean) * rstd);
        }
    const float inv_d = 1.f / (float)D;
    const float mg = MODE == MODE_LN ? group_sum<LPR>(sg) * inv_d : 0.f;
    const float mgx = group_sum<LPR>(sgx) * inv_d;
    if (!live) return;
    float* dr = dx + row * D;
    for (int d = sub; d < D; d += LPR) {
        const float g = w ? gr[d] * w[d] : gr[d];
        dr[d] = rstd * (g - mg - (xr[d] - mean) * rstd * mgx);
    }
}

// stage one of dweight / dbias: block (cb, p) sums rows [p * RB, (p + 1) * RB) of columns cb*64 .. cb*64+63; its four waves take the
// rows in turn and meet in LDS in wave order.  part_w / part_b: [nparts][D]
template <int MODE>
__global__ __launch_bounds__(256) void rownorm_bwd_wb_part_k(const float* __restrict__ dy, const float* __restrict__ x,
                                                             const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                             float* __restrict__ part_w, float* __restrict__ part_b, long rows, int D, int RB) {
    __shared__ float shw[4][64], shb[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int d = blockIdx.x * 64 + lane;
    const long r0 = (long)blockIdx.y * RB, r1 = r0 + RB < rows ? r0 + RB : rows;
    float sw = 0.f, sb = 0.f;
    if (d < D)
        for (long r = r0 + wave; r < r1; r += 4) {
            const float g = dy[r * D + d];
            const float mean = MODE == MODE_LN ? mean_in[r] : 0.f;
            sw += g * ((x[r * D + d] - mean) * rstd_in[r]);
            sb += g;
        }
    shw[wave][lane] = sw;
    shb[wave][lane] = sb;
    __syncthreads();
    if (wave == 0 && d < D) {
        if (part_w) part_w[(long)blockIdx.y * D + d] = ((shw[0][lane] + shw[1][lane]) + shw[2][lane]) + shw[3][lane];
        if (part_b) part_b[(long)blockIdx.y * D + d] = ((shb[0][lane] + shb[1][lane]) + shb[2][lane]) + shb[3][lane];
    }
}

// stage two: out[d] = part[0][d] + part[1][d] + ... in order
__global__ __launch_bounds__(256) void fold_parts_k(const float* __restrict__ part, float* __restrict__ out, int nparts, int D) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    float s = 0.f;
    for (int p = 0; p < nparts; ++p) s += part[(long)p * D + d];
    out[d] = s;
}

constexpr float RSQRT2 = 0.70710678118654752440f, RSQRT2PI = 0.39894228040143267794f;

// y = gelu(x + b[col]), gelu(z) = z * 0.5 * (1 + erf(z / sqrt(2)))  (nn.GELU() default: approximate="none")
__global__ __launch_bounds__(256) void bias_gelu_fwd_k(const float* __restrict__ x, const float* __restrict__ b, float* __restrict__ y, long n, int c) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
        const float z = b ? x[t] + b[t % c] : x[t];
        y[t] = z * 0.5f * (1.f + erff(z * RSQRT2));
    }
}

// dx = dy * (Phi(z) + z * phi(z)), z = x + b[col] recomputed from the saved pre-bias x
__global__ __launch_bounds__(256) void bias_gelu_bwd_k(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ b,
                                                       float* __restrict__ dx, long n, int c) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
        const float z = b ? x[t] + b[t % c] : x[t];
        const float cdf = 0.5f * (1.f + erff(z * RSQRT2));
        const float pdf = expf(-0.5f * z * z) * RSQRT2PI;
        dx[t] = dy[t] * (cdf + z * pdf);
    }
}

// Unpatchify + tanh.  One thread per OUTPUT element (b, y, x, c) of the NHWC image; its source is token (y / p) * (W / p) + x / p,
// channel ((y % p) * p + x % p) * C + c.  BWD: din at the source = dout * (1 - out^2)
template <bool BWD>
__global__ __launch_bounds__(256) void unpatchify_act_k(const float* __restrict__ src, const float* __restrict__ saved, float* __restrict__ dst,
                                                        long n, int H, int W, int C, int p) {
    const int wt = W / p;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
        const int c = (int)(t % C);
        long r = t / C;
        const int xx = (int)(r % W);
        r /= W;
        const int yy = (int)(r % H);
        const long b = r / H;
        const long tok = (b * (H / p) + yy / p) * wt + xx / p;
        const long at = tok * ((long)p * p * C) + ((long)(yy % p) * p + xx % p) * C + c;
        if (BWD) {
            const float o = saved[t];
            dst[at] = src[t] * (1.f - o * o);
        } else {
            dst[t] = tanhf(src[at]);
        }
    }
}

// y[row][d] = x[row][d] + pos[row % period][d]
__global__ __launch_bounds__(256) void add_rows_bcast_k(const float* __restrict__ x, const float* __restrict__ pos, float* __restrict__ y, long n,
                                                        long pn) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) y[t] = x[t] + pos[t % pn];
}

unsigned grid1d(long n) {
    long g = (n + 255) / 256;
    return (unsigned)(g > 16384 ? 16384 : (g < 1 ? 1 : g));
}

int rownorm_parts(long rows, int* rb) {
    // at most 256 partial rows, each over at least 32 rows
    long per = (rows + 255) / 256;
    if (per < 32) per = 32;
    *rb = (int)per;
    return (int)((rows + per - 1) / per);
}

}  // namespace

extern "C" {

int movae_rownorm_fwd(const float* x, const float* weight, const float* bias, const float* pos, int pos_rows, float* out, float* mean,
                      float* rstd, long rows, int d, int mode, float eps, movae_stream_t stream) {
    MOVAE_CHECK_ARG(x && out && rstd && rows > 0 && d > 0, "movae_rownorm_fwd: bad argument");
    MOVAE_CHECK_ARG(mode == MODE_LN || mode == MODE_RMS, "movae_rownorm_fwd: mode must be 0 (LayerNorm) or 1 (RMSNorm), got %d", mode);
    MOVAE_CHECK_ARG(mode != MODE_LN || mean, "movae_rownorm_fwd: LayerNorm saves the row means (mean is null)");
    MOVAE_CHECK_ARG(mode != MODE_RMS || !bias, "movae_rownorm_fwd: RMSNorm has no bias");
    MOVAE_CHECK_ARG(!pos || pos_rows > 0, "movae_rownorm_fwd: pos needs its row count");
    MOVAE_CHECK_ARG(rows <= (1L << 40) / d, "movae_rownorm_fwd: sizes out of range");
    const hipStream_t s = (hipStream_t)stream;
    const int period = pos ? pos_rows : 1;
#define ROWNORM_FWD(LPR, MODE)                                                                                                      \
    hipLaunchKernelGGL((rownorm_fwd_k<LPR, MODE>), dim3((unsigned)((rows + 256 / LPR - 1) / (256 / LPR))), dim3(256), 0, s, x, weight, bias, \
                       pos, out, mean, rstd, rows, d, period, eps)
    if (d <= 32) {
        if (mode == MODE_LN) ROWNORM_FWD(8, MODE_LN);
        else ROWNORM_FWD(8, MODE_RMS);
    } else {
        if (mode == MODE_LN) ROWNORM_FWD(64, MODE_LN);
        else ROWNORM_FWD(64, MODE_RMS);
    }
#undef ROWNORM_FWD
    MOVAE_CHECK_LAUNCH("rownorm_fwd");
    return MOVAE_OK;
}

size_t movae_rownorm_ws_bytes(long rows, int d) {
    int rb;
    const int np = rownorm_parts(rows, &rb);
    return MOVAE_WS_HEADER_BYTES + (size_t)2 * np * d * sizeof(float);
}

int movae_rownorm_bwd(const float* dy, const float* x, const float* weight, const float* mean, const float* rstd, float* dx, float* dweight,
                      float* dbias, long rows, int d, int mode, void* ws, size_t ws_bytes, movae_stream_t stream) {
    MOVAE_WS_SCRATCH(ws, ws_bytes);
    MOVAE_CHECK_ARG(dy && x && rstd && rows > 0 && d > 0, "movae_rownorm_bwd: bad argument");
    MOVAE_CHECK_ARG(mode == MODE_LN || mode == MODE_RMS, "movae_rownorm_bwd: mode must be 0 (LayerNorm) or 1 (RMSNorm), got %d", mode);
    MOVAE_CHECK_ARG(mode != MODE_LN || mean, "movae_rownorm_bwd: LayerNorm needs the saved row means");
    MOVAE_CHECK_ARG(mode != MODE_RMS || !dbias, "movae_rownorm_bwd: RMSNorm has no bias");
    MOVAE_CHECK_ARG(dx || dweight || dbias, "movae_rownorm_bwd: nothing to compute");
    MOVAE_CHECK_ARG(rows <= (1L << 40) / d, "movae_rownorm_bwd: sizes out of range");
    const hipStream_t s = (hipStream_t)stream;
    if (dx) {
#define ROWNORM_BWD(LPR, MODE)                                                                                                          \
    hipLaunchKernelGGL((rownorm_bwd_dx_k<LPR, MODE>), dim3((unsigned)((rows + 256 / LPR - 1) / (256 / LPR))), dim3(256), 0, s, dy, x, weight, \
                       mean, rstd, dx, rows, d)
        if (d <= 32) {
            if (mode == MODE_LN) ROWNORM_BWD(8, MODE_LN);
            else ROWNORM_BWD(8, MODE_RMS);
        } else {
            if (mode == MODE_LN) ROWNORM_BWD(64, MODE_LN);
            else ROWNORM_BWD(64, MODE_RMS);
        }
#undef ROWNORM_BWD
        MOVAE_CHECK_LAUNCH("rownorm_bwd_dx");
    }
    if (dweight || dbias) {
        int rb;
        const int np = rownorm_parts(rows, &rb);
        MOVAE_CHECK_ARG(ws && ws_bytes >= (size_t)2 * np * d * sizeof(float), "movae_rownorm_bwd: workspace too small");
        float* pw = dweight ? static_cast<float*>(ws) : nullptr;
        float* pb = dbias ? static_cast<float*>(ws) + (size_t)np * d : nullptr;
        const dim3 grid((unsigned)((d + 63) / 64), (unsigned)np);
        if (mode == MODE_LN)
            hipLaunchKernelGGL(rownorm_bwd_wb_part_k<MODE_LN>, grid, dim3(256), 0, s, dy, x, mean, rstd, pw, pb, rows, d, rb);
        else
            hipLaunchKernelGGL(rownorm_bwd_wb_part_k<MODE_RMS>, grid, dim3(256), 0, s, dy, x, mean, rstd, pw, pb, rows, d, rb);
        MOVAE_CHECK_LAUNCH("rownorm_bwd_wb_part");
        if (dweight) hipLaunchKernelGGL(fold_parts_k, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, pw, dweight, np, d);
        if (dbias) hipLaunchKernelGGL(fold_parts_k, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, pb, dbias, np, d);
        MOVAE_CHECK_LAUNCH("rownorm_bwd_fold");
    }
    return MOVAE_OK;
}

int movae_bias_gelu_fwd(const float* x, const float* bias, float* y, long rows, int c, movae_stream_t stream) {
    MOVAE_CHECK_ARG(x && y && rows > 0 && c > 0, "movae_bias_gelu_fwd: bad argument");
    const long n = rows * c;
    hipLaunchKernelGGL(bias_gelu_fwd_k, dim3(grid1d(n)), dim3(256), 0, (hipStream_t)stream, x, bias, y, n, c);
    MOVAE_CHECK_LAUNCH("bias_gelu_fwd");
    return MOVAE_OK;
}

int movae_bias_gelu_bwd(const float* dy, const float* x, const float* bias, float* dx, long rows, int c, movae_stream_t stream) {
    MOVAE_CHECK_ARG(dy && x && dx && rows > 0 && c > 0, "movae_bias_gelu_bwd: bad argument");
    const long n = rows * c;
    hipLaunchKernelGGL(bias_gelu_bwd_k, dim3(grid1d(n)), dim3(256), 0, (hipStream_t)stream, dy, x, bias, dx, n, c);
    MOVAE_CHECK_LAUNCH("bias_gelu_bwd");
    return MOVAE_OK;
}

int movae_unpatchify_act_fwd(const float* x, float* out, int b, int h, int w, int c, int patch, movae_stream_t stream) {
    MOVAE_CHECK_ARG(x && out && b > 0 && h > 0 && w > 0 && c > 0 && patch > 0, "movae_unpatchify_act_fwd: bad argument");
    MOVAE_CHECK_ARG(h % patch == 0 && w % patch == 0, "movae_unpatchify_act_fwd: image %dx%d is no multiple of the patch %d", h, w, patch);
    const long n = (long)b * h * w * c;
    hipLaunchKernelGGL(unpatchify_act_k<false>, dim3(grid1d(n)), dim3(256), 0, (hipStream_t)stream, x, (const float*)nullptr, out, n, h, w, c,
                       patch);
    MOVAE_CHECK_LAUNCH("unpatchify_act_fwd");
    return MOVAE_OK;
}

int movae_unpatchify_act_bwd(const float* dout, const float* out, float* dx, int b, int h, int w, int c, int patch, movae_stream_t stream) {
    MOVAE_CHECK_ARG(dout && out && dx && b > 0 && h > 0 && w > 0 && c > 0 && patch > 0, "movae_unpatchify_act_bwd: bad argument");
    MOVAE_CHECK_ARG(h % patch == 0 && w % patch == 0, "movae_unpatchify_act_bwd: image %dx%d is no multiple of the patch %d", h, w, patch);
    const long n = (long)b * h * w * c;
    hipLaunchKernelGGL(unpatchify_act_k<true>, dim3(grid1d(n)), dim3(256), 0, (hipStream_t)stream, dout, out, dx, n, h, w, c, patch);
    MOVAE_CHECK_LAUNCH("unpatchify_act_bwd");
    return MOVAE_OK;
}

int movae_add_rows_bcast(const float* x, const float* pos, float* y, long rows, int pos_rows, int d, movae_stream_t stream) {
    MOVAE_CHECK_ARG(x && pos && y && rows > 0 && pos_rows > 0 && d > 0, "movae_add_rows_bcast: bad argument");
    MOVAE_CHECK_ARG(rows % pos_rows == 0, "movae_add_rows_bcast: %ld rows are no multiple of the table's %d", rows, pos_rows);
    const long n = rows * d;
    hipLaunchKernelGGL(add_rows_bcast_k, dim3(grid1d(n)), dim3(256), 0, (hipStream_t)stream, x, pos, y, n, (long)pos_rows * d);
    MOVAE_CHECK_LAUNCH("add_rows_bcast");
    return MOVAE_OK;
}

}  // extern "C"
