// Element-wise / layout kernels (all HBM-bound; 16-byte accesses wherever alignment allows).
#include "common.h"

namespace {

inline int grid_for(long total, int per = 256) {
    long g = (total + per - 1) / per;
    return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

inline bool al16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

// per image: src [R][Cc] -> dst [Cc][R]  (batched 2-D transpose through a padded LDS tile)
__global__ __launch_bounds__(256) void transpose_batched(const float* __restrict__ src, float* __restrict__ dst, int R, int Cc) {
    __shared__ float tile[32][33];
    const long img = blockIdx.z;
    const float* s = src + img * (long)R * Cc;
    float* d = dst + img * (long)R * Cc;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
    for (int i = 0; i < 32; i += 8) {
        const int r = r0 + ty + i, c = c0 + tx;
        if (r < R && c < Cc) tile[ty + i][tx] = s[(long)r * Cc + c];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 32; i += 8) {
        const int c = c0 + ty + i, r = r0 + tx;
        if (r < R && c < Cc) d[(long)c * R + r] = tile[tx][ty + i];
    }
}

// the input batch: [N][3][HW] -> [N][HW][3].  A 32 x 32 transpose tile uses 3 of its 32 rows here (1.4 TB/s at C5); a thread takes
// four consecutive pixels instead: one 16-byte load per plane, three 16-byte stores (HW % 4 == 0, 16-byte aligned: host).
__global__ __launch_bounds__(256) void nchw3_to_nhwc_k(const float* __restrict__ src, float* __restrict__ dst, long quads_per_img,
                                                      long total_quads) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total_quads; q += stride) {
        const long img = q / quads_per_img, k = q - img * quads_per_img;
        const float* s = src + img * quads_per_img * 12 + k * 4;
        const f32x4 r = *reinterpret_cast<const f32x4*>(s), g = *reinterpret_cast<const f32x4*>(s + quads_per_img * 4),
                    b = *reinterpret_cast<const f32x4*>(s + quads_per_img * 8);
        f32x4* d = reinterpret_cast<f32x4*>(dst + q * 12);
        d[0] = f32x4{r[0], g[0], b[0], r[1]};
        d[1] = f32x4{g[1], b[1], r[2], g[2]};
        d[2] = f32x4{b[2], r[3], g[3], b[3]};
    }
}

template <bool VEC>
__global__ void act_fwd_k(const float* __restrict__ x, float* __restrict__ y, long n, int act, float slope) {
    const long stride = (long)gridDim.x * blockDim.x;
    if (VEC) {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += stride) {
            f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = apply_act(v[j], act, slope);
            reinterpret_cast<f32x4*>(y)[i] = v;
        }
    } else {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = apply_act(x[i], act, slope);
    }
}

template <bool VEC>
__global__ void act_bwd_k(const float* __restrict__ dy, const float* __restrict__ out, float* __restrict__ dx, long n,
                          int act, float slope) {
    const long stride = (long)gridDim.x * blockDim.x;
    if (VEC) {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += stride) {
            const f32x4 g = reinterpret_cast<const f32x4*>(dy)[i];
            const f32x4 o = reinterpret_cast<const f32x4*>(out)[i];
            f32x4 r;
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = g[j] * act_grad_from_out(o[j], act, slope);
            reinterpret_cast<f32x4*>(dx)[i] = r;
        }
    } else {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
            dx[i] = dy[i] * act_grad_from_out(out[i], act, slope);
    }
}

// `groups` stacked cotangents of one forward: out is shared, blockIdx.y = group (n4 = float4 quads per group)
__global__ void act_bwd_grouped_k(const float* __restrict__ dy, const float* __restrict__ out, float* __restrict__ dx, long n4,
                                  int act, float slope) {
    const long stride = (long)gridDim.x * blockDim.x, off = (long)blockIdx.y * n4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f32x4 g = reinterpret_cast<const f32x4*>(dy)[off + i];
        const f32x4 o = reinterpret_cast<const f32x4*>(out)[i];
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = g[j] * act_grad_from_out(o[j], act, slope);
        reinterpret_cast<f32x4*>(dx)[off + i] = r;
    }
}

template <bool VEC>
__global__ void axpby_k(float alpha, const float* __restrict__ a, float beta, const float* __restrict__ b,
                        float* __restrict__ y, long n) {
    const long stride = (long)gridDim.x * blockDim.x;
    if (VEC) {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += stride) {
            const f32x4 u = reinterpret_cast<const f32x4*>(a)[i];
            const f32x4 v = reinterpret_cast<const f32x4*>(b)[i];
            reinterpret_cast<f32x4*>(y)[i] = alpha * u + beta * v;
        }
    } else {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = alpha * a[i] + beta * b[i];
    }
}

__global__ void copy_channels_k(const float* __restrict__ src, float* __restrict__ dst, long rows, int c_src, int c_dst,
                                int src_off, int dst_off, int c_copy) {
    const long total = rows * c_copy;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long r = i / c_copy;
        const int c = (int)(i - r * c_copy);
        dst[r * c_dst + dst_off + c] = src[r * c_src + src_off + c];
    }
}

// column sums, two-stage fp64
__global__ __launch_bounds__(256) void colsum_partial(const float* __restrict__ x, double* __restrict__ part, int rows, int C,
                                                      int CB, int rows_per_block) {
    __shared__ double sh[256];
    const int t = threadIdx.x;
    const int RG = 256 / CB;
    const int cl = t % CB, rg = t / CB;
    const long r0 = (long)blockIdx.x * rows_per_block;
    const long r1 = min((long)rows, r0 + rows_per_block);
    for (int cb = 0; cb < C; cb += CB) {
        const int c = cb + cl;
        double s = 0.0;
        if (c < C)
            for (long r = r0 + rg; r < r1; r += RG) s += x[r * C + c];
        sh[t] = s;
        __syncthreads();
        if (rg == 0 && c < C) {
            for (int i = 1; i < RG; ++i) s += sh[i * CB + cl];
            part[(long)blockIdx.x * C + c] = s;
        }
        __syncthreads();
    }
}

// 16-byte variant: a thread owns one 4-channel quad (C % 4 == 0), a wave reads 1 KiB contiguous
__global__ __launch_bounds__(256) void colsum_partial4(const float* __restrict__ x, double* __restrict__ part, int rows,
                                                       int C, int CQB, int rows_per_block) {
    __shared__ double sh[4 * 256];
    const int t = threadIdx.x, RG = 256 / CQB, cl = t % CQB, rg = t / CQB, CQ = C / 4;
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min((long)rows, r0 + rows_per_block);
    for (int cb = 0; cb < CQ; cb += CQB) {
        const int cq = cb + cl;
        double v[4] = {0, 0, 0, 0};
        if (cq < CQ)
            for (long r = r0 + rg; r < r1; r += 4 * RG) {
                f32x4 a[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long rr = r + (long)u * RG;
                    a[u] = rr < r1 ? *reinterpret_cast<const f32x4*>(x + rr * C + cq * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] += (double)a[u][j];
            }
        fold_columns_256<4>(v, sh, CQB);
        if (rg == 0 && cq < CQ) {
#pragma unroll
            for (int j = 0; j < 4; ++j) part[(long)blockIdx.x * C + cq * 4 + j] = v[j];
        }
    }
}

// ---- activation backward fused with the bias gradient --------------------------------------------------------------
// dpre = dy * act'(y) and, in the same pass, the per-channel sums of dpre (the bias gradient of the conv that produced y).
// Without the fusion the column-sum kernel re-reads dpre: on the bias + LeakyReLU stacks (BetaTC-VAE, VQ-VAE-2) that
// pass and its launch pair were ~5 % of the step.  grid = (row blocks, cotangent groups); y is shared by the groups.
struct BiasOut {
    float* p[8];
};

__global__ __launch_bounds__(256) void act_bwd_colsum4(const float* __restrict__ dy, const float* __restrict__ y,
                                                       float* __restrict__ dpre, double* __restrict__ part, int rows, int C, int CQB,
                                                       int rows_per_block, int act, float slope) {
    __shared__ double sh[4 * 256];
    const long gs = (long)rows * C;
    dy += blockIdx.y * gs;
    dpre += blockIdx.y * gs;
    part += (long)blockIdx.y * gridDim.x * C;
    const int t = threadIdx.x, RG = 256 / CQB, cl = t % CQB, rg = t / CQB, CQ = C / 4;
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min((long)rows, r0 + rows_per_block);
    for (int cb = 0; cb < CQ; cb += CQB) {
        const int cq = cb + cl;
        double v[4] = {0, 0, 0, 0};
        if (cq < CQ)
            for (long r = r0 + rg; r < r1; r += 4 * RG) {
                f32x4 g4[4], y4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long rr = r + (long)u * RG;
                    if (rr < r1) {
                        g4[u] = *reinterpret_cast<const f32x4*>(dy + rr * C + cq * 4);
                        y4[u] = *reinterpret_cast<const f32x4*>(y + rr * C + cq * 4);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long rr = r + (long)u * RG;
                    if (rr < r1) {
                        f32x4 o;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            o[j] = g4[u][j] * act_grad_from_out(y4[u][j], act, slope);
                            v[j] += (double)o[j];
                        }
                        *reinterpret_cast<f32x4*>(dpre + rr * C + cq * 4) = o;
                    }
                }
            }
        fold_columns_256<4>(v, sh, CQB);
        if (rg == 0 && cq < CQ) {
#pragma unroll
            for (int j = 0; j < 4; ++j) part[(long)blockIdx.x * C + cq * 4 + j] = v[j];
        }
    }
}

__global__ __launch_bounds__(64) void colsum_final_grouped(const double* __restrict__ part, int nblk, int C, BiasOut out, int accumulate) {
    const int c = blockIdx.x;
    part += (long)blockIdx.y * nblk * C;
    float* __restrict__ dst = out.p[blockIdx.y];
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) s += part[(long)b * C + c];
    s = wave_sum(s);
    if (threadIdx.x == 0 && dst) dst[c] = accumulate ? dst[c] + (float)s : (float)s;
}

__global__ __launch_bounds__(64) void colsum_final(const double* __restrict__ part, int nblk, int C, float* __restrict__ out,
                                                   int accumulate) {
    const int c = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) s += part[(long)b * C + c];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[c] = accumulate ? out[c] + (float)s : (float)s;
}

__global__ void reparam_fwd_k(const float* __restrict__ mu, const float* __restrict__ lv, const float* __restrict__ eps,
                              float* __restrict__ z, long n) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) z[i] = mu[i] + eps[i] * expf(0.5f * lv[i]);
}

// ---- reparameterisation with the noise drawn in the kernel --------------------------------------------------------------------
// torch.randn_like inside a captured hipGraph costs three launches per replay (two Philox state updates and the generator kernel)
// in front of this 5 us op.  Here the standard normal eps is drawn from Philox4x32-10 (Salmon et al., SC'11; the generator family
// torch / cuRAND / rocRAND use) keyed by `seed`, one counter block (quad index, draw number) per four outputs, Box-Muller on the
// four words.  state[0] = seed, state[1] = number of draws made so far: read by every block, advanced by the block that finishes
// last (g_reparam_done), so a replayed graph draws fresh noise every time.  eps is written out for the backward.
__device__ unsigned g_reparam_done = 0;

// quads [0, ceil(n / 4)) draw eps (and z); with `prior`, the quads that follow draw prior[0 .. n_prior) -- the cycle branch's
// z_prior of the recursive-cyclic VAEs -- from the same draw number: one launch and one counter advance for both
__global__ __launch_bounds__(256) void reparam_rng_fwd_k(const float* __restrict__ mu, const float* __restrict__ lv, float* __restrict__ eps,
                                                         float* __restrict__ z, long n, float* __restrict__ prior, long n_prior,
                                                         unsigned long long* __restrict__ state, int advance) {
    const unsigned long long seed = state[0], draw = state[1];
    const long nq = (n + 3) / 4, nq_all = nq + (prior ? (n_prior + 3) / 4 : 0), stride = (long)gridDim.x * blockDim.x;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq_all; q += stride) {
        float e[4];
        normal4(q, draw, seed, e);
        if (q < nq) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long i = q * 4 + j;
                if (i < n) {
                    eps[i] = e[j];
                    z[i] = mu[i] + e[j] * expf(0.5f * lv[i]);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long i = (q - nq) * 4 + j;
                if (i < n_prior) prior[i] = e[j];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned done = atomicAdd(&g_reparam_done, 1u);
        if (done == gridDim.x - 1) {
            g_reparam_done = 0;
            if (advance) state[1] = draw + 1;
        }
    }
}

__global__ void reparam_bwd_k(const float* __restrict__ dz, const float* __restrict__ lv, const float* __restrict__ eps,
                              float* __restrict__ dmu, float* __restrict__ dlv, long n) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float g = dz[i];
        dmu[i] = g;
        dlv[i] = g * eps[i] * expf(0.5f * lv[i]) * 0.5f;
    }
}

inline int pow2_ge(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace

extern "C" {

int movae_nchw_to_nhwc(const float* src, float* dst, int n, int c, int h, int w, movae_stream_t stream) {
    MOVAE_CHECK_ARG(src && dst && n > 0 && c > 0 && h > 0 && w > 0, "movae_nchw_to_nhwc: bad argument");
    const int R = c, Cc = h * w;  // per image [C][HW] -> [HW][C]
    if (c == 3 && Cc % 4 == 0 && al16(src, dst)) {
        const long qpi = Cc / 4, total = qpi * n;
        long gq = (total + 255) / 256;
        if (gq > 8192) gq = 8192;
        hipLaunchKernelGGL(nchw3_to_nhwc_k, dim3((unsigned)gq), dim3(256), 0, (hipStream_t)stream, src, dst, qpi, total);
        MOVAE_CHECK_LAUNCH("nchw3_to_nhwc");
        return MOVAE_OK;
    }
    dim3 grid(ceil_div(Cc, 32), ceil_div(R, 32), n);
    hipLaunchKernelGGL(transpose_batched, grid, dim3(256), 0, (hipStream_t)stream, src, dst, R, Cc);
    MOVAE_CHECK_LAUNCH("transpose_batched");
    return MOVAE_OK;
}

int movae_nhwc_to_nchw(const float* src, float* dst, int n, int c, int h, int w, movae_stream_t stream) {
    MOVAE_CHECK_ARG(src && dst && n > 0 && c > 0 && h > 0 && w > 0, "movae_nhwc_to_nchw: bad argument");
    const int R = h * w, Cc = c;  // per image [HW][C] -> [C][HW]
    dim3 grid(ceil_div(Cc, 32), ceil_div(R, 32), n);
    hipLaunchKernelGGL(transpose_batched, grid, dim3(256), 0, (hipStream_t)stream, src, dst, R, Cc);
    MOVAE_CHECK_LAUNCH("transpose_batched");
    return MOVAE_OK;
}

int movae_act_fwd(const float* x, float* y, size_t n, int act, float slope, movae_stream_t stream) {
    MOVAE_CHECK_ARG(x && y && n > 0, "movae_act_fwd: bad argument");
    if (n % 4 == 0 && al16(x, y))
        hipLaunchKernelGGL(act_fwd_k<true>, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, x, y, (long)n, act, slope);
    else
        hipLaunchKernelGGL(act_fwd_k<false>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, y, (long)n, act, slope);
    MOVAE_CHECK_LAUNCH("act_fwd");
    return MOVAE_OK;
}

int movae_act_bwd(const float* dy, const float* out, float* dx, size_t n, int act, float slope, movae_stream_t stream) {
    MOVAE_CHECK_ARG(dy && out && dx && n > 0, "movae_act_bwd: bad argument");
    if (n % 4 == 0 && al16(dy, out, dx))
        hipLaunchKernelGGL(act_bwd_k<true>, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, dy, out, dx, (long)n, act, slope);
    else
        hipLaunchKernelGGL(act_bwd_k<false>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, dy, out, dx, (long)n, act, slope);
    MOVAE_CHECK_LAUNCH("act_bwd");
    return MOVAE_OK;
}

int movae_axpby(float alpha, const float* a, float beta, const float* b, float* y, size_t n, movae_stream_t stream) {
    MOVAE_CHECK_ARG(a && b && y && n > 0, "movae_axpby: bad argument");
    if (n % 4 == 0 && al16(a, b, y))
        hipLaunchKernelGGL(axpby_k<true>, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, alpha, a, beta, b, y, (long)n);
    else
        hipLaunchKernelGGL(axpby_k<false>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, alpha, a, beta, b, y, (long)n);
    MOVAE_CHECK_LAUNCH("axpby");
    return MOVAE_OK;
}

int movae_add(const float* a, const float* b, float* y, size_t n, movae_stream_t stream) {
    return movae_axpby(1.f, a, 1.f, b, y, n, stream);
}

int movae_copy_channels(const float* src, float* dst, int rows, int c_src, int c_dst, int src_off, int dst_off, int c_copy,
                        movae_stream_t stream) {
    MOVAE_CHECK_ARG(src && dst && rows > 0 && c_copy > 0 && src_off >= 0 && dst_off >= 0 && src_off + c_copy <= c_src &&
                        dst_off + c_copy <= c_dst,
                    "movae_copy_channels: bad argument");
    hipLaunchKernelGGL(copy_channels_k, dim3(grid_for((long)rows * c_copy)), dim3(256), 0, (hipStream_t)stream, src, dst,
                       (long)rows, c_src, c_dst, src_off, dst_off, c_copy);
    MOVAE_CHECK_LAUNCH("copy_channels");
    return MOVAE_OK;
}

int movae_act_bwd_bias_grouped(int groups, const float* dy, const float* out, float* dpre, float* const* dbias, int rows, int c,
                               int act, float slope, int accumulate, void* ws, size_t ws_bytes, movae_stream_t stream) {
    MOVAE_WS_SCRATCH(ws, ws_bytes);
    MOVAE_CHECK_ARG(dy && out && dpre && rows > 0 && c > 0 && groups >= 1 && groups <= 8, "movae_act_bwd_bias: bad argument");
    MOVAE_CHECK_ARG(c % 4 == 0 && al16(dy, out, dpre), "movae_act_bwd_bias: needs c %% 4 == 0 and 16-byte aligned tensors");
    if (!dbias) {  // no bias gradient wanted here (the weight-gradient kernel sums dpre itself): the grouped activation backward alone
        const long n4 = (long)rows * c / 4;
        hipLaunchKernelGGL(act_bwd_grouped_k, dim3(grid_for(n4), groups), dim3(256), 0, (hipStream_t)stream, dy, out, dpre, n4, act, slope);
        MOVAE_CHECK_LAUNCH("act_bwd_grouped");
        return MOVAE_OK;
    }
    const int cq = c / 4;
    const int CQB = pow2_ge(cq) < 256 ? pow2_ge(cq) : 256;
    const int RG4 = 256 / CQB;
    int rpb4 = ceil_div(rows, 512);
    rpb4 = ceil_div(rpb4, RG4) * RG4;
    if (rpb4 < RG4 * 4) rpb4 = RG4 * 4;
    const int nblk = ceil_div(rows, rpb4);
    MOVAE_CHECK_ARG(ws && ws_bytes >= (size_t)groups * nblk * c * sizeof(double), "movae_act_bwd_bias: workspace too small");
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(act_bwd_colsum4, dim3(nblk, groups), dim3(256), 0, (hipStream_t)stream, dy, out, dpre, part, rows, c, CQB, rpb4,
                       act, slope);
    MOVAE_CHECK_LAUNCH("act_bwd_colsum4");
    BiasOut tab;
    for (int i = 0; i < 8; ++i) tab.p[i] = i < groups ? dbias[i] : nullptr;
    hipLaunchKernelGGL(colsum_final_grouped, dim3(c, groups), dim3(64), 0, (hipStream_t)stream, part, nblk, c, tab, accumulate);
    MOVAE_CHECK_LAUNCH("colsum_final_grouped");
    return MOVAE_OK;
}

int movae_colsum(const float* x, float* out, int rows, int c, int accumulate, void* ws, size_t ws_bytes, movae_stream_t stream) {
    MOVAE_WS_SCRATCH(ws, ws_bytes);
    MOVAE_CHECK_ARG(x && out && rows > 0 && c > 0, "movae_colsum: bad argument");
    if (c % 4 == 0 && al16(x) && ws) {
        const int cq = c / 4;
        const int CQB = pow2_ge(cq) < 256 ? pow2_ge(cq) : 256;
        const int RG4 = 256 / CQB;
        int rpb4 = ceil_div(rows, 256);
        rpb4 = ceil_div(rpb4, RG4) * RG4;
        if (rpb4 < RG4 * 8) rpb4 = RG4 * 8;
        const int nblk4 = ceil_div(rows, rpb4);
        MOVAE_CHECK_ARG(ws && ws_bytes >= (size_t)nblk4 * c * sizeof(double), "movae_colsum: workspace too small");
        double* part4 = static_cast<double*>(ws);
        hipLaunchKernelGGL(colsum_partial4, dim3(nblk4), dim3(256), 0, (hipStream_t)stream, x, part4, rows, c, CQB, rpb4);
        MOVAE_CHECK_LAUNCH("colsum_partial4");
        hipLaunchKernelGGL(colsum_final, dim3(c), dim3(64), 0, (hipStream_t)stream, part4, nblk4, c, out, accumulate);
        MOVAE_CHECK_LAUNCH("colsum_final");
        return MOVAE_OK;
    }
    const int CB = pow2_ge(c) < 256 ? pow2_ge(c) : 256;
    const int RG = 256 / CB;
    int rpb = ceil_div(rows, 256);
    rpb = ceil_div(rpb, RG) * RG;
    if (rpb < RG * 4) rpb = RG * 4;
    const int nblk = ceil_div(rows, rpb);
    MOVAE_CHECK_ARG(ws && ws_bytes >= (size_t)nblk * c * sizeof(double), "movae_colsum: workspace too small");
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(colsum_partial, dim3(nblk), dim3(256), 0, (hipStream_t)stream, x, part, rows, c, CB, rpb);
    MOVAE_CHECK_LAUNCH("colsum_partial");
    hipLaunchKernelGGL(colsum_final, dim3(c), dim3(64), 0, (hipStream_t)stream, part, nblk, c, out, accumulate);
    MOVAE_CHECK_LAUNCH("colsum_final");
    return MOVAE_OK;
}

int movae_reparam_fwd(const float* mu, const float* log_var, const float* eps, float* z, size_t n, movae_stream_t stream) {
    MOVAE_CHECK_ARG(mu && log_var && eps && z && n > 0, "movae_reparam_fwd: bad argument");
    hipLaunchKernelGGL(reparam_fwd_k, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, mu, log_var, eps, z, (long)n);
    MOVAE_CHECK_LAUNCH("reparam_fwd");
    return MOVAE_OK;
}

int movae_reparam_rng_fwd(const float* mu, const float* log_var, float* eps, float* z, size_t n, unsigned long long* state, int advance,
                          movae_stream_t stream) {
    MOVAE_CHECK_ARG(mu && log_var && eps && z && state && n > 0, "movae_reparam_rng_fwd: bad argument");
    hipLaunchKernelGGL(reparam_rng_fwd_k, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, mu, log_var, eps, z, (long)n,
                       (float*)nullptr, 0L, state, advance);
    MOVAE_CHECK_LAUNCH("reparam_rng_fwd");
    return MOVAE_OK;
}

int movae_reparam_prior_rng_fwd(const float* mu, const float* log_var, float* eps, float* z, size_t n, float* prior, size_t n_prior,
                                unsigned long long* state, int advance, movae_stream_t stream) {
    MOVAE_CHECK_ARG(mu && log_var && eps && z && prior && state && n > 0 && n_prior > 0, "movae_reparam_prior_rng_fwd: bad argument");
    hipLaunchKernelGGL(reparam_rng_fwd_k, dim3(grid_for((n + 3) / 4 + (n_prior + 3) / 4)), dim3(256), 0, (hipStream_t)stream, mu, log_var,
                       eps, z, (long)n, prior, (long)n_prior, state, advance);
    MOVAE_CHECK_LAUNCH("reparam_prior_rng_fwd");
    return MOVAE_OK;
}

int movae_reparam_bwd(const float* dz, const float* log_var, const float* eps, float* dmu, float* dlog_var, size_t n,
                      movae_stream_t stream) {
    MOVAE_CHECK_ARG(dz && log_var && eps && dmu && dlog_var && n > 0, "movae_reparam_bwd: bad argument");
    hipLaunchKernelGGL(reparam_bwd_k, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, dz, log_var, eps, dmu, dlog_var, (long)n);
    MOVAE_CHECK_LAUNCH("reparam_bwd");
    return MOVAE_OK;
}

}  // extern "C"
