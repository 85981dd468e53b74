// The conv Sphere Encoder (models/sphere_encoder.py): the arithmetic between its encoder and decoder passes and its three losses.
//
//   sphere_latents   v = n(z), v_noisy = n(v + sigma e), v_noisy_small = n(v + sigma_sub e) with n(x) = radius x / sqrt(mean(x^2) + eps),
//                    the jitter-angle schedule (sigma = tan(angle), sigma_sub = s sigma) and, in graph mode, the draws themselves:
//                    one launch where the reference makes about thirty.  One row of z / e per wave (L <= 512) or per block, read
//                    once and held in registers; every row sum is a fixed-order fp32 fold (lane-serial, xor butterfly, then the
//                    waves of the block in index order), so a rerun is bit-identical.
//   sphere_losses    pix_recon, pix_con, lat_con and their sum in two launches (partials, final) reading `recons` once for both
//                    pixel terms; fp64 partials like losses.hip.
//
// Row layout of the latent kernels: thread t of the NT that share a row owns the quads t, t + NT, ... (elements 4q .. 4q + 3), loaded
// as one 16-byte access when L % 4 == 0 and the bases are 16-byte aligned, else as four guarded scalar accesses (L = 6, 12, 130, 2051:
// the row pitch breaks the alignment, and the last quad is partial).
#include "common.h"

namespace {

constexpr float DEG2RAD = 0.017453292519943295f;

template <int RQ>
struct Row {
    float a[RQ * 4];
};

template <int NT, int RQ, bool VEC>
__device__ __forceinline__ void row_load(Row<RQ>& r, const float* __restrict__ p, int L, int t) {
#pragma unroll
    for (int k = 0; k < RQ; ++k) {
        const int i = 4 * (t + k * NT);
        if (VEC) {
            const float4 q = i < L ? *reinterpret_cast<const float4*>(p + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            r.a[4 * k] = q.x, r.a[4 * k + 1] = q.y, r.a[4 * k + 2] = q.z, r.a[4 * k + 3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) r.a[4 * k + j] = i + j < L ? p[i + j] : 0.f;
        }
    }
}

template <int NT, int RQ, bool VEC>
__device__ __forceinline__ void row_store(const Row<RQ>& r, float* __restrict__ p, int L, int t) {
#pragma unroll
    for (int k = 0; k < RQ; ++k) {
        const int i = 4 * (t + k * NT);
        if (VEC) {
            if (i < L) *reinterpret_cast<float4*>(p + i) = make_float4(r.a[4 * k], r.a[4 * k + 1], r.a[4 * k + 2], r.a[4 * k + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i + j < L) p[i + j] = r.a[4 * k + j];
        }
    }
}

// sum over the row's NT threads, the same value in each of them; sh: NT / 64 floats per value, used when NT > 64
template <int NT, int NV>
__device__ __forceinline__ void row_sum(float (&s)[NV], float* sh) {
#pragma unroll
    for (int q = 0; q < NV; ++q) s[q] = wave_sum(s[q]);
    if (NT > 64) {
        constexpr int NW = NT / 64;
        const int w = threadIdx.x >> 6;
        __syncthreads();  // (the previous fold's readers are done with sh)
        if ((threadIdx.x & 63) == 0)
#pragma unroll
            for (int q = 0; q < NV; ++q) sh[q * NW + w] = s[q];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            float a = sh[q * NW];
            for (int i = 1; i < NW; ++i) a += sh[q * NW + i];
            s[q] = a;
        }
    }
}

__device__ unsigned g_sphere_done = 0;

struct LatArgs {
    const float* z;
    float* e;             // read (given) or written (drawn); null: the clean projection only
    float* u;             // [B][4] angle, mix mask, mix angle, s: read or written; null with a given sigma
    const float* sig_in;  // given sigma: per row (sig_rows) or one scalar read from sig_in[0]; null: sig_val when fixed
    float sig_val;
    int fixed, sig_rows;
    unsigned long long* state;  // draw e and u in the launch from {seed, draws}
    int advance;
    int B, L;
    float angle_max, mix_prob, mix_min, mix_max, radius, eps;
    float *v, *vn, *vs, *sigma, *sigma_sub, *inv;  // outputs, each nullable; inv: [3][B]
};

template <int NT, int RQ, bool VEC>
__global__ __launch_bounds__(NT < 256 ? 256 : NT) void sphere_latents_fwd_k(LatArgs a) {
    __shared__ float sh[2 * 16];
    constexpr int RPB = NT < 256 ? 256 / NT : 1;  // rows per block
    const int t = NT < 256 ? (threadIdx.x & (NT - 1)) : threadIdx.x;
    const int row = blockIdx.x * RPB + (NT < 256 ? threadIdx.x / NT : 0);
    const int L = a.L;
    const float invL = 1.f / (float)L;
    unsigned long long seed = 0, draw = 0;
    if (a.state) seed = a.state[0], draw = a.state[1];
    if (row < a.B) {  // (wave-uniform: a row never shares a wave)
        const long base = (long)row * L;
        Row<RQ> z, e;
        row_load<NT, RQ, VEC>(z, a.z + base, L, t);
        float s1[1] = {0.f};
#pragma unroll
        for (int k = 0; k < RQ * 4; ++k) s1[0] += z.a[k] * z.a[k];
        row_sum<NT, 1>(s1, sh);
        const float rms_z = sqrtf(s1[0] * invL + a.eps);  // (x / rms) * radius, the reference's element-wise operations in its order
#pragma unroll
        for (int k = 0; k < RQ * 4; ++k) z.a[k] = (z.a[k] / rms_z) * a.radius;  // z holds v from here on
        if (a.v) row_store<NT, RQ, VEC>(z, a.v + base, L, t);
        if (a.inv && t == 0) a.inv[row] = 1.f / rms_z;
        if (a.e) {
            const int nq = (L + 3) / 4;
            const long q0 = (long)row * (nq + 1);  // the row's counter blocks: nq of e, then one of u
            float u4[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.state) {
#pragma unroll
                for (int k = 0; k < RQ; ++k) {
                    const int q = t + k * NT;
                    float n4[4] = {0.f, 0.f, 0.f, 0.f};
                    if (q < nq) normal4(q0 + q, draw, seed, n4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) e.a[4 * k + j] = 4 * q + j < L ? n4[j] : 0.f;
                }
                row_store<NT, RQ, VEC>(e, a.e + base, L, t);
                unsigned w[4];
                const long qu = q0 + nq;
                philox4x32_10((unsigned)qu, (unsigned)((unsigned long long)qu >> 32), (unsigned)draw, (unsigned)(draw >> 32), (unsigned)seed,
                              (unsigned)(seed >> 32), w);
#pragma unroll
                for (int j = 0; j < 4; ++j) u4[j] = unit_open(w[j]);
                if (a.u && t == 0)
#pragma unroll
                    for (int j = 0; j < 4; ++j) a.u[(long)row * 4 + j] = u4[j];
            } else {
                row_load<NT, RQ, VEC>(e, a.e + base, L, t);
                if (!a.fixed)
#pragma unroll
                    for (int j = 0; j < 4; ++j) u4[j] = a.u[(long)row * 4 + j];
            }
            float sg, sgs = 0.f;
            if (a.fixed) {
                sg = a.sig_in ? a.sig_in[a.sig_rows ? row : 0] : a.sig_val;
            } else {
                float deg = u4[0] * a.angle_max;
                if (a.mix_prob > 0.f && u4[1] < a.mix_prob) deg = a.mix_min + u4[2] * (a.mix_max - a.mix_min);
                sg = tanf(deg * DEG2RAD);
                sgs = (0.5f * u4[3]) * sg;
            }
            if (t == 0) {
                if (a.sigma) a.sigma[row] = sg;
                if (a.sigma_sub) a.sigma_sub[row] = sgs;
            }
            const bool small = a.vs != nullptr;
            float s2[2] = {0.f, 0.f};
#pragma unroll
            for (int k = 0; k < RQ * 4; ++k) {
                const float w = z.a[k] + sg * e.a[k], ws = z.a[k] + sgs * e.a[k];
                s2[0] += w * w;
                s2[1] += ws * ws;
            }
            row_sum<NT, 2>(s2, sh);
            const float rms_n = sqrtf(s2[0] * invL + a.eps), rms_s = sqrtf(s2[1] * invL + a.eps);
            if (a.inv && t == 0) {
                a.inv[a.B + row] = 1.f / rms_n;
                if (small) a.inv[2 * a.B + row] = 1.f / rms_s;
            }
            Row<RQ> o;
            if (a.vn) {
#pragma unroll
                for (int k = 0; k < RQ * 4; ++k) o.a[k] = ((z.a[k] + sg * e.a[k]) / rms_n) * a.radius;
                row_store<NT, RQ, VEC>(o, a.vn + base, L, t);
            }
            if (small) {
#pragma unroll
                for (int k = 0; k < RQ * 4; ++k) o.a[k] = ((z.a[k] + sgs * e.a[k]) / rms_s) * a.radius;
                row_store<NT, RQ, VEC>(o, a.vs + base, L, t);
            }
        }
    }
    if (a.state) {  // the block that finishes last advances the draw number (every block has read it by then)
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned done = atomicAdd(&g_sphere_done, 1u);
            if (done == gridDim.x - 1) {
                g_sphere_done = 0;
                if (a.advance) a.state[1] = draw + 1;
            }
        }
    }
}

struct LatBwdArgs {
    const float *v, *e, *sigma, *sigma_sub, *inv;  // e / sigma / sigma_sub nullable with the cotangents that need them
    const float *g_v, *g_n, *g_s;                  // nullable
    float* dz;
    int B, L;
    float radius;
};

// dz = nT(g_v + nT(g_n; w) + nT(g_s; w'); z),  nT(g; x) = radius (g / rms - x (g . x) / (L rms^3)),  w = v + sigma e,  w' = v + sigma_sub e
template <int NT, int RQ, bool VEC>
__global__ __launch_bounds__(NT < 256 ? 256 : NT) void sphere_latents_bwd_k(LatBwdArgs a) {
    __shared__ float sh[2 * 16];
    constexpr int RPB = NT < 256 ? 256 / NT : 1;
    const int t = NT < 256 ? (threadIdx.x & (NT - 1)) : threadIdx.x;
    const int row = blockIdx.x * RPB + (NT < 256 ? threadIdx.x / NT : 0);
    if (row >= a.B) return;  // (no block-wide barrier follows for NT < 256; for NT >= 256 the whole block leaves)
    const int L = a.L;
    const float invL = 1.f / (float)L;
    const long base = (long)row * L;
    Row<RQ> v, h;
    row_load<NT, RQ, VEC>(v, a.v + base, L, t);
    if (a.g_v) {
        row_load<NT, RQ, VEC>(h, a.g_v + base, L, t);
    } else {
#pragma unroll
        for (int k = 0; k < RQ * 4; ++k) h.a[k] = 0.f;
    }
    if (a.g_n || a.g_s) {
        Row<RQ> e, gn, gs;
        row_load<NT, RQ, VEC>(e, a.e + base, L, t);
        const float sg = a.g_n ? a.sigma[row] : 0.f, sgs = a.g_s ? a.sigma_sub[row] : 0.f;
        const float inv_n = a.g_n ? a.inv[a.B + row] : 0.f, inv_s = a.g_s ? a.inv[2 * a.B + row] : 0.f;
        float d[2] = {0.f, 0.f};
        if (a.g_n) {
            row_load<NT, RQ, VEC>(gn, a.g_n + base, L, t);
#pragma unroll
            for (int k = 0; k < RQ * 4; ++k) d[0] += gn.a[k] * (v.a[k] + sg * e.a[k]);
        }
        if (a.g_s) {
            row_load<NT, RQ, VEC>(gs, a.g_s + base, L, t);
#pragma unroll
            for (int k = 0; k < RQ * 4; ++k) d[1] += gs.a[k] * (v.a[k] + sgs * e.a[k]);
        }
        row_sum<NT, 2>(d, sh);
        const float cn = d[0] * invL * inv_n * inv_n * inv_n, cs = d[1] * invL * inv_s * inv_s * inv_s;
        if (a.g_n)
#pragma unroll
            for (int k = 0; k < RQ * 4; ++k) h.a[k] += a.radius * (gn.a[k] * inv_n - (v.a[k] + sg * e.a[k]) * cn);
        if (a.g_s)
#pragma unroll
            for (int k = 0; k < RQ * 4; ++k) h.a[k] += a.radius * (gs.a[k] * inv_s - (v.a[k] + sgs * e.a[k]) * cs);
    }
    // z = v / (radius inv_z):  z (h . z) / (L rms^3) = v (h . v) inv_z / (radius^2 L)
    const float inv_z = a.inv[row];
    float c[1] = {0.f};
#pragma unroll
    for (int k = 0; k < RQ * 4; ++k) c[0] += h.a[k] * v.a[k];
    row_sum<NT, 1>(c, sh);
    const float cz = c[0] * invL / (a.radius * a.radius);
#pragma unroll
    for (int k = 0; k < RQ * 4; ++k) h.a[k] = (a.radius * inv_z) * (h.a[k] - v.a[k] * cz);
    row_store<NT, RQ, VEC>(h, a.dz + base, L, t);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the instantiation for a row length: a wave per row up to 512, a block of 256 up to 4096, of 1024 up to 16384
template <typename A, typename F64, typename F256, typename F1024>
inline int launch_rows(const char* name, const A& a, int B, int L, bool vec, hipStream_t st, F64 k64, F256 k256, F1024 k1024) {
    if (L <= 512) {
        hipLaunchKernelGGL(k64[vec], dim3((B + 3) / 4), dim3(256), 0, st, a);
    } else if (L <= 4096) {
        hipLaunchKernelGGL(k256[vec], dim3(B), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(k1024[vec], dim3(B), dim3(1024), 0, st, a);
    }
    MOVAE_CHECK_LAUNCH(name);
    return MOVAE_OK;
}

constexpr int MAX_L = 16384;

// ---- losses ---------------------------------------------------------------------------------------------------------------------
constexpr int RED_BLOCKS = 1024;

inline int red_blocks(size_t n) {
    size_t g = (n + 1023) / 1024;
    return (int)(g > RED_BLOCKS ? RED_BLOCKS : (g < 1 ? 1 : g));
}

__device__ __forceinline__ float sl1(float d) {  // smooth-L1, beta = 1 (losses.hip: MOVAE_RECON_SMOOTH_L1)
    d = fabsf(d);
    return d < 1.f ? 0.5f * d * d : d - 0.5f;
}
__device__ __forceinline__ float dsl1(float d) { return fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : -1.f); }

// (ab, aa, bb) of one latent row, fp64 lane sums folded over the wave
__device__ __forceinline__ void cos_sums(const float* __restrict__ p, const float* __restrict__ q, int L, int lane, double& ab, double& aa,
                                         double& bb) {
    ab = aa = bb = 0.0;
    for (int i = lane; i < L; i += 64) {
        const double x = p[i], y = q[i];
        ab += x * y, aa += x * x, bb += y * y;
    }
    ab = wave_sum(ab), aa = wave_sum(aa), bb = wave_sum(bb);
}

// blocks [0, nb1): partial sums of smooth_l1(r - x) -> part[blk] and smooth_l1(xn - tgt) -> part[nb1 + blk], tgt = sg or, when sg is
// null, the r just read (three image tensors in one pass); blocks [nb1, ..): one wave per latent row, 1 - cos -> part[2 nb1 + row]
__global__ __launch_bounds__(256) void sphere_partial(const float* __restrict__ r, const float* __restrict__ x, const float* __restrict__ xn,
                                                      const float* __restrict__ sg, long n, const float* __restrict__ v,
                                                      const float* __restrict__ ve, int B, int L, int nb1, double* __restrict__ part) {
    __shared__ double sh[4];
    const int blk = (int)blockIdx.x;
    if (blk < nb1) {
        double s = 0.0, c = 0.0;
        const long stride = (long)nb1 * 256;
        for (long i = (long)blk * 256 + threadIdx.x; i < n; i += stride) {
            const float ri = r[i];
            s += sl1(ri - x[i]);
            c += sl1(xn[i] - (sg ? sg[i] : ri));
        }
        s = block_sum_256(s, sh);
        c = block_sum_256(c, sh);
        if (threadIdx.x == 0) part[blk] = s, part[nb1 + blk] = c;
    } else {
        const int row = (blk - nb1) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (row >= B) return;
        double ab, aa, bb;
        cos_sums(v + (long)row * L, ve + (long)row * L, L, lane, ab, aa, bb);
        const double na = fmax(sqrt(aa), 1e-8), nb = fmax(sqrt(bb), 1e-8);  // F.cosine_similarity eps
        if (lane == 0) part[2 * nb1 + row] = 1.0 - (double)(float)(ab / (na * nb));
    }
}

// out = [lam_rec (w_rs mean), lam_con (w_cs mean), lam_lat mean_b(1 - cos), their fp32 sum in that order]
__global__ __launch_bounds__(256) void sphere_final(const double* __restrict__ part, int nb1, long n, int B, float lam_rec, float w_rs,
                                                    float lam_con, float w_cs, float lam_lat, float* __restrict__ out) {
    __shared__ double sh[4];
    double s = 0.0, c = 0.0, l = 0.0;
    for (int i = threadIdx.x; i < nb1; i += 256) s += part[i], c += part[nb1 + i];
    for (int i = threadIdx.x; i < B; i += 256) l += part[2 * nb1 + i];
    s = block_sum_256(s, sh);
    c = block_sum_256(c, sh);
    l = block_sum_256(l, sh);
    if (threadIdx.x != 0) return;
    const float rec = lam_rec * (w_rs * (float)(s / (double)n)), con = lam_con * (w_cs * (float)(c / (double)n));
    const float lat = lam_lat * (float)(l / (double)B);
    out[0] = rec, out[1] = con, out[2] = lat, out[3] = (rec + con) + lat;
}

__device__ __forceinline__ float cot2(const float* a, const float* t) { return (a ? a[0] : 0.f) + (t ? t[0] : 0.f); }

// blocks [0, nb1): drecons = f_rec smooth_l1'(r - x) (pix_con treats recons as a constant), dxn = f_con smooth_l1'(xn - tgt);
// blocks [nb1, ..): one wave per latent row, dv / dve of lam_lat mean_b(1 - cos)
__global__ __launch_bounds__(256) void sphere_losses_bwd_k(const float* __restrict__ r, const float* __restrict__ x, const float* __restrict__ xn,
                                                           const float* __restrict__ sg, long n, const float* __restrict__ v,
                                                           const float* __restrict__ ve, int B, int L, int nb1, float f_rec, float f_con,
                                                           float f_lat, const float* __restrict__ g_rec, const float* __restrict__ g_con,
                                                           const float* __restrict__ g_lat, const float* __restrict__ g_tot,
                                                           float* __restrict__ dr, float* __restrict__ dxn, float* __restrict__ dv,
                                                           float* __restrict__ dve) {
    const int blk = (int)blockIdx.x;
    if (blk < nb1) {
        const float fr = f_rec * cot2(g_rec, g_tot), fc = f_con * cot2(g_con, g_tot);
        const long stride = (long)nb1 * 256;
        for (long i = (long)blk * 256 + threadIdx.x; i < n; i += stride) {
            const float ri = r[i];
            if (dr) dr[i] = fr * dsl1(ri - x[i]);
            if (dxn) dxn[i] = fc * dsl1(xn[i] - (sg ? sg[i] : ri));
        }
    } else {
        const int row = (blk - nb1) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (row >= B) return;
        const float* p = v + (long)row * L;
        const float* q = ve + (long)row * L;
        double ab, aa, bb;
        cos_sums(p, q, L, lane, ab, aa, bb);
        const double na = fmax(sqrt(aa), 1e-8), nb = fmax(sqrt(bb), 1e-8);
        // d cos / dp = q / (na nb) - p ab / (na^3 nb) (the second term absent while the norm sits at its clamp), and likewise for q
        const double f = -(double)(f_lat * cot2(g_lat, g_tot)), inn = 1.0 / (na * nb);
        const double ca = na > 1e-8 ? ab * inn / (na * na) : 0.0, cb = nb > 1e-8 ? ab * inn / (nb * nb) : 0.0;
        for (int i = lane; i < L; i += 64) {
            const double pi = p[i], qi = q[i];
            if (dv) dv[(long)row * L + i] = (float)(f * (qi * inn - pi * ca));
            if (dve) dve[(long)row * L + i] = (float)(f * (pi * inn - qi * cb));
        }
    }
}

inline int grid_el(long n) {
    long g = (n + 255) / 256;
    return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}
}  // namespace

extern "C" {

int movae_sphere_latents_fwd(const float* z, float* e, float* u, const float* sigma_in, int sigma_rows, float sigma_val, int fixed_sigma,
                             unsigned long long* state, int advance, int b, int l, float angle_max_deg, float mix_prob, float mix_min_deg,
                             float mix_max_deg, float radius, float eps, float* v, float* v_noisy, float* v_noisy_small, float* sigma,
                             float* sigma_sub, float* inv_rms, movae_stream_t stream) {
    MOVAE_CHECK_ARG(z && b > 0 && l > 0, "movae_sphere_latents_fwd: bad argument");
    MOVAE_CHECK_ARG(l <= MAX_L, "movae_sphere_latents_fwd: rows longer than %d are not supported (got %d)", MAX_L, l);
    MOVAE_CHECK_ARG(e || !(v_noisy || v_noisy_small || state || u), "movae_sphere_latents_fwd: the noisy projections need e");
    MOVAE_CHECK_ARG(!e || fixed_sigma || u, "movae_sphere_latents_fwd: the angle schedule needs u (given, or drawn into)");
    MOVAE_CHECK_ARG(!(state && fixed_sigma), "movae_sphere_latents_fwd: a given sigma takes a given e");
    MOVAE_CHECK_ARG(!(fixed_sigma && v_noisy_small), "movae_sphere_latents_fwd: a given sigma produces v_noisy only");
    MOVAE_CHECK_ARG(v || v_noisy || v_noisy_small, "movae_sphere_latents_fwd: no output");
    LatArgs a{z, e, u, sigma_in, sigma_val, fixed_sigma, sigma_rows, state, advance, b, l, angle_max_deg, mix_prob, mix_min_deg, mix_max_deg,
              radius, eps, v, v_noisy, v_noisy_small, sigma, sigma_sub, inv_rms};
    const bool vec = l % 4 == 0 && aligned16(z) && aligned16(e) && aligned16(v) && aligned16(v_noisy) && aligned16(v_noisy_small);
    void (*k64[2])(LatArgs) = {sphere_latents_fwd_k<64, 2, false>, sphere_latents_fwd_k<64, 2, true>};
    void (*k256[2])(LatArgs) = {sphere_latents_fwd_k<256, 4, false>, sphere_latents_fwd_k<256, 4, true>};
    void (*k1024[2])(LatArgs) = {sphere_latents_fwd_k<1024, 4, false>, sphere_latents_fwd_k<1024, 4, true>};
    return launch_rows("sphere_latents_fwd", a, b, l, vec, (hipStream_t)stream, k64, k256, k1024);
}

int movae_sphere_latents_bwd(const float* v, const float* e, const float* sigma, const float* sigma_sub, const float* inv_rms,
                             const float* g_v, const float* g_noisy, const float* g_small, float* dz, int b, int l, float radius,
                             movae_stream_t stream) {
    MOVAE_CHECK_ARG(v && inv_rms && dz && b > 0 && l > 0, "movae_sphere_latents_bwd: bad argument");
    MOVAE_CHECK_ARG(l <= MAX_L, "movae_sphere_latents_bwd: rows longer than %d are not supported (got %d)", MAX_L, l);
    MOVAE_CHECK_ARG(g_v || g_noisy || g_small, "movae_sphere_latents_bwd: no cotangent");
    MOVAE_CHECK_ARG(!g_noisy || (e && sigma), "movae_sphere_latents_bwd: g_noisy needs e and sigma");
    MOVAE_CHECK_ARG(!g_small || (e && sigma_sub), "movae_sphere_latents_bwd: g_small needs e and sigma_sub");
    LatBwdArgs a{v, e, sigma, sigma_sub, inv_rms, g_v, g_noisy, g_small, dz, b, l, radius};
    const bool vec = l % 4 == 0 && aligned16(v) && aligned16(e) && aligned16(g_v) && aligned16(g_noisy) && aligned16(g_small) && aligned16(dz);
    void (*k64[2])(LatBwdArgs) = {sphere_latents_bwd_k<64, 2, false>, sphere_latents_bwd_k<64, 2, true>};
    void (*k256[2])(LatBwdArgs) = {sphere_latents_bwd_k<256, 4, false>, sphere_latents_bwd_k<256, 4, true>};
    void (*k1024[2])(LatBwdArgs) = {sphere_latents_bwd_k<1024, 4, false>, sphere_latents_bwd_k<1024, 4, true>};
    return launch_rows("sphere_latents_bwd", a, b, l, vec, (hipStream_t)stream, k64, k256, k1024);
}

size_t movae_sphere_losses_ws_bytes(size_t n, int b) {
    return MOVAE_WS_HEADER_BYTES + ((size_t)2 * red_blocks(n) + (size_t)(b > 0 ? b : 0)) * sizeof(double);
}

int movae_sphere_losses_fwd(const float* recons, const float* inputs, const float* x_noisy, const float* recons_sg, size_t n, const float* v,
                            const float* v_enc_dec, int b, int l, float lam_rec, float w_rec_sl1, float lam_con, float w_con_sl1,
                            float lam_lat, float* out, void* ws, size_t ws_bytes, movae_stream_t stream) {
    MOVAE_CHECK_ARG(ws && ws_bytes >= movae_sphere_losses_ws_bytes(n, b), "movae_sphere_losses_fwd: workspace too small");
    MOVAE_WS_SCRATCH(ws, ws_bytes);
    MOVAE_CHECK_ARG(recons && inputs && x_noisy && v && v_enc_dec && out && n > 0 && b > 0 && l > 0, "movae_sphere_losses_fwd: bad argument");
    const int nb1 = red_blocks(n), nb2 = (b + 3) / 4;
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(sphere_partial, dim3(nb1 + nb2), dim3(256), 0, (hipStream_t)stream, recons, inputs, x_noisy, recons_sg, (long)n, v,
                       v_enc_dec, b, l, nb1, part);
    MOVAE_CHECK_LAUNCH("sphere_partial");
    hipLaunchKernelGGL(sphere_final, dim3(1), dim3(256), 0, (hipStream_t)stream, part, nb1, (long)n, b, lam_rec, w_rec_sl1, lam_con, w_con_sl1,
                       lam_lat, out);
    MOVAE_CHECK_LAUNCH("sphere_final");
    return MOVAE_OK;
}

int movae_sphere_losses_bwd(const float* recons, const float* inputs, const float* x_noisy, const float* recons_sg, size_t n, const float* v,
                            const float* v_enc_dec, int b, int l, float lam_rec, float w_rec_sl1, float lam_con, float w_con_sl1,
                            float lam_lat, const float* g_rec, const float* g_con, const float* g_lat, const float* g_tot, float* drecons,
                            float* dx_noisy, float* dv, float* dv_enc_dec, movae_stream_t stream) {
    MOVAE_CHECK_ARG(recons && inputs && x_noisy && v && v_enc_dec && n > 0 && b > 0 && l > 0, "movae_sphere_losses_bwd: bad argument");
    MOVAE_CHECK_ARG(drecons || dx_noisy || dv || dv_enc_dec, "movae_sphere_losses_bwd: no output");
    const int nb1 = (drecons || dx_noisy) ? grid_el((long)n) : 0, nb2 = (dv || dv_enc_dec) ? (b + 3) / 4 : 0;
    hipLaunchKernelGGL(sphere_losses_bwd_k, dim3(nb1 + nb2), dim3(256), 0, (hipStream_t)stream, recons, inputs, x_noisy, recons_sg, (long)n, v,
                       v_enc_dec, b, l, nb1, lam_rec * w_rec_sl1 / (float)n, lam_con * w_con_sl1 / (float)n, lam_lat / (float)b, g_rec, g_con,
                       g_lat, g_tot, drecons, dx_noisy, dv, dv_enc_dec);
    MOVAE_CHECK_LAUNCH("sphere_losses_bwd");
    return MOVAE_OK;
}

}  // extern "C"
