// Shared helpers for the gfx950 kernels (wave64, fp32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/movae.h"

#define MOVAE_OK 0
#define MOVAE_EINVAL (-1)
#define MOVAE_EUNSUPPORTED (-2)
#define MOVAE_ELAUNCH (-3)

void movae_set_error(const char* fmt, ...);

// movae_set_compute_dtype(): 1 = bf16 MFMA operands (fp32 accumulate) in the 128x128 implicit-GEMM kernels (conv_igemm.hip, which
// defines it) and in the attention kernels (attention.hip); 0 = fp32, the default and the parity path
extern int g_movae_compute_bf16;

#define MOVAE_CHECK_ARG(cond, ...)            \
    do {                                      \
        if (!(cond)) {                        \
            movae_set_error(__VA_ARGS__);     \
            return MOVAE_EINVAL;              \
        }                                     \
    } while (0)

#define MOVAE_CHECK_LAUNCH(name)                                                     \
    do {                                                                             \
        hipError_t e_ = hipGetLastError();                                           \
        if (e_ != hipSuccess) {                                                      \
            movae_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));   \
            return MOVAE_ELAUNCH;                                                    \
        }                                                                            \
    } while (0)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

static inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// an environment switch / tuning threshold: its value where set, else the default (INTEGRATION.md lists every name)
static inline long env_long(const char* name, long dflt) {
    const char* v = getenv(name);
    return v ? atol(v) : dflt;
}
static inline double env_double(const char* name, double dflt) {
    const char* v = getenv(name);
    return v ? atof(v) : dflt;
}

__device__ __forceinline__ float apply_act(float v, int act, float slope) {
    switch (act) {
        case MOVAE_ACT_LRELU: return v > 0.f ? v : v * slope;
        case MOVAE_ACT_RELU: return v > 0.f ? v : 0.f;
        case MOVAE_ACT_TANH: return tanhf(v);
        case MOVAE_ACT_SIGMOID: return 1.f / (1.f + expf(-v));
        default: return v;
    }
}

// derivative of the activation expressed through its OUTPUT value
__device__ __forceinline__ float act_grad_from_out(float o, int act, float slope) {
    switch (act) {
        case MOVAE_ACT_LRELU: return o > 0.f ? 1.f : slope;
        case MOVAE_ACT_RELU: return o > 0.f ? 1.f : 0.f;
        case MOVAE_ACT_TANH: return 1.f - o * o;
        case MOVAE_ACT_SIGMOID: return o * (1.f - o);
        default: return 1.f;
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- workspace header ----------------------------------------------------------------------------------
// The first MOVAE_WS_HEADER_BYTES of a caller's workspace are reserved and zero on first use; no kernel uses them
// at present.
#define MOVAE_WS_HEADER_BYTES 4096

// plain-scratch users skip the header so it stays zero
#define MOVAE_WS_SCRATCH(ws, ws_bytes)                                         \
    do {                                                                       \
        if ((ws) && (ws_bytes) > (size_t)MOVAE_WS_HEADER_BYTES) {              \
            (ws) = static_cast<char*>(ws) + MOVAE_WS_HEADER_BYTES;             \
            (ws_bytes) -= MOVAE_WS_HEADER_BYTES;                               \
        } else {                                                               \
            (ws) = nullptr;                                                    \
            (ws_bytes) = 0;                                                    \
        }                                                                      \
    } while (0)

// Philox4x32-10 (Salmon et al., SC'11; the counter-based generator family torch / cuRAND / rocRAND use): four 32-bit words of
// counter (c0..c3) under key (k0, k1).  Shared by the reparameterisation draws (eltwise.hip) and the attention dropout mask
// (attention.hip); unit_open / normal4 below turn its words into the uniforms and standard normals of the in-kernel noise draws
// (eltwise.hip, sphere.hip).
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

__device__ __forceinline__ float unit_open(unsigned x) { return ((float)(x >> 8) + 0.5f) * (1.f / 16777216.f); }  // (0, 1), 24 bits

// four standard normals of counter block (quad q, draw number): the Philox words through Box-Muller
__device__ __forceinline__ void normal4(long q, unsigned long long draw, unsigned long long seed, float e[4]) {
    unsigned w[4];
    philox4x32_10((unsigned)q, (unsigned)((unsigned long long)q >> 32), (unsigned)draw, (unsigned)(draw >> 32), (unsigned)seed,
                  (unsigned)(seed >> 32), w);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float r = sqrtf(-2.f * logf(unit_open(w[2 * h]))), t = 6.28318530717958647692f * unit_open(w[2 * h + 1]);
        float sn, cs;
        sincosf(t, &sn, &cs);
        e[2 * h] = r * cs, e[2 * h + 1] = r * sn;
    }
}

// block-wide sum for 256-thread blocks; result valid in every thread
// Column fold of a 256-thread block whose thread t owns column cl = t % CQB of row group rg = t / CQB (CQB a power of two):
// on return the threads with rg == 0 hold, in v[], the sums over all row groups of their column.  Row groups that share a
// wave are folded with shuffles first, so the serial part is at most 4 LDS reads per value (the naive form made the
// 256 / CQB row groups a serial loop on CQB threads -- 32 deep for a 32-channel tensor).  sh: NV * 256 doubles.
template <int NV>
__device__ __forceinline__ void fold_columns_256(double (&v)[NV], double* sh, int CQB) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (CQB < 64) {
        for (int off = CQB; off < 64; off <<= 1)
#pragma unroll
            for (int q = 0; q < NV; ++q) v[q] += __shfl_xor(v[q], off, 64);
        if (lane < CQB)
#pragma unroll
            for (int q = 0; q < NV; ++q) sh[q * 256 + wave * 64 + lane] = v[q];
        __syncthreads();
        if (t < CQB)
#pragma unroll
            for (int q = 0; q < NV; ++q)
                v[q] = (sh[q * 256 + t] + sh[q * 256 + 64 + t]) + (sh[q * 256 + 128 + t] + sh[q * 256 + 192 + t]);
    } else {
#pragma unroll
        for (int q = 0; q < NV; ++q) sh[q * 256 + t] = v[q];
        __syncthreads();
        if (t < CQB) {
            const int RG = 256 / CQB;
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                double s = v[q];
                for (int i = 1; i < RG; ++i) s += sh[q * 256 + i * CQB + t];
                v[q] = s;
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ double block_sum_256(double v, double* sh /* >= 4 doubles */) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}
