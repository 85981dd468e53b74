// Fused causal multi-head self-attention of PixelSNAIL's CausalAttention2d (reference models/pixelcnn_prior.py:95-135):
// S = Q K^T / sqrt(hd), causal mask j <= i (diagonal included, :16-22), softmax, dropout on the probabilities, O = P' V.
// FlashAttention-2 form: the [L, L] matrix never exists.  The forward keeps an online softmax over 16-key tiles and saves the
// log-sum-exp; the backward recomputes P from it in two passes without float atomics -- one per 16-key tile (dK, dV) and one per
// 16-query tile (dQ) -- so every gradient is bit-identical from run to run.
//
// Layout.  q / k / v are the 1x1-conv outputs [B, L, ld] (NHWC, ld >= heads * hd); head h is channels h*hd .. h*hd+hd-1, read in
// place.  O and dO are [B, L, heads * hd] in the reference's channel order d*heads + h (out.permute(0, 2, 3, 1).reshape, :130).
// dq / dk / dv are written in the q / k / v layout (same ld).
//
// Math.  fp32 in, fp32 accumulate on v_mfma_f32_16x16x4_f32 (gfx950 has no xf32).  One wave owns a 16-row tile; lane l holds
// column c = l & 15 and row group g = l >> 4 of every 16x16 fragment (C/D: col = c, row = 4g + reg).  The products are oriented so
// that the softmax row of a query lives on the 4 lanes {c, c+16, c+32, c+48}:
//   forward / dQ:  S^T = K Q^T  (lane c: query i0+c; reg r: key j0+4g+r),  O^T += V^T P^T,  dQ^T += K^T dS^T
//   dK / dV:       S   = Q K^T  (lane c: key j0+c;   reg r: query i0+4g+r), dV^T += dO^T P', dK^T += Q^T dS
// and the second product of each pair takes the first one's accumulator registers as its B operand directly: its k-step r uses the
// key (query) set {4g + r}, which is the same set on both operands.  The head dim is padded to HDP in {8, 16, 32, 64} with masked
// loads; the QK^T k-steps use d = g * HDP/4 + s, so each lane group reads a contiguous run of a row.
//
// Dropout.  keep(bh, i, j) = word (j & 3) of Philox4x32-10 at counter (j >> 2, i, bh, draw_lo), key (seed_lo, seed_hi ^ draw_hi),
// kept iff the word < thr = (1 - p) * 2^32.  A pure function of (seed, draw, bh, i, j): the forward, both backward passes and
// movae_causal_attn_dropout_mask regenerate the same mask whatever their tiling.
//
// The bidirectional form (movae_attn_*: AttentionWithRoPE of models/sphere_encoder_vit.py:143-167) is the same three kernels with
// CAUSAL off -- every query sees every key j < L, all tiles in both loops, no dropout instances -- the head-major output order
// h*hd + d (out strides oh / od), and optionally RoPE: q and k are rotated as they are loaded, pair t of a row at position n by
// the angle whose cos / sin the host tabulated at [n][t]; (u[2t], u[2t+1]) -> (u[2t] c - u[2t+1] s, u[2t] s + u[2t+1] c).  The pair
// partner of an element is in the same lane for the g*NS + s loads (NS is even) and in lane c ^ 1 for the cc*16 + c loads; dq / dk
// come out as gradients of the ROTATED rows and are rotated back (the transpose rotation) in registers before the store.
//
// bf16 operands (movae_set_compute_dtype(MOVAE_DTYPE_BF16): attn_fwd_bf_k, attn_bwd_dkdv_bf_k, attn_bwd_dq_bf_k; every hd <= 64 and
// every causal / dropout / RoPE combination takes them in that mode -- no shape stays on the fp32 instances).  Same entry points, HBM
// layouts, workspace, tile-to-wave map, orientation and masks; v_mfma_f32_16x16x32_bf16, whose C/D map is the fp32 form's.  Rounded
// to bf16 (RNE, __builtin_convertvector): q and k AFTER RoPE, v, dO, the probabilities after the dropout scaling, and dS with its
// 1 / sqrt(hd).  fp32: accumulation, the logits' scale, the running max, the row sum (of the UNROUNDED probabilities), lse, delta
// (attn_delta_k as it is), dP - delta and the rotation back of dq / dk.  The loop step is 32 keys (queries in dK / dV): two 16-row
// first products whose 2 x 4 accumulator registers, converted pairwise, are the B operand of ONE 32-deep second product.  k slot
// (g, e) of that step is position 16 (e >> 2) + 4 g + (e & 3), so the A operand (V^T, K^T; dO^T, Q^T) is read from a TRANSPOSED
// LDS image [d][position] as the two 4-position runs at 4 g and 16 + 4 g.  Each step's tiles are staged once per block, as bf16,
// and shared by the four waves: a row image [32][HDP + 8] (d contiguous; the A operand of the first products, one ds_read_b128 per
// lane) and a transposed image [16 NC][36] (the second products), both written from registers that were loaded a step ahead.
// RoPE is applied between the global load and the LDS store.  Every wave reaches both barriers of every step: waves whose tile lies
// beyond L, or (causal) beyond the diagonal for this step, skip only the arithmetic.  The head dim is covered by NC = 1 / 2 / 4
// chunks of 16 output columns and padded to HDP = 32 / 32 / 64 in the reduction.
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

struct AttnArgs {
    const float* q;
    const float* k;
    const float* v;
    const float* dout;
    const float* lse;
    const float* delta;
    float* out;
    float* lse_out;
    float* dq;
    float* dk;
    float* dv;
    const float* cos;  // RoPE tables [L][hd / 2] (ROPE instances only)
    const float* sin;
    long ld;       // row stride of q / k / v / dq / dk / dv (floats)
    int oh, od;    // out / dout: element (h, d) of a row at h * oh + d * od
    int heads, L, hd, ntiles, nbh;
    float scale;   // 1 / sqrt(hd)
    unsigned thr;  // keep iff Philox word < thr (and p > 0)
    int drop;
    float inv_keep;
    unsigned s0, s1, d0;  // Philox key (seed lo, seed hi ^ draw hi) and counter word 3 (draw lo)
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ void keep4(const AttnArgs& a, int bh, int i, int jq, unsigned w[4]) {
    philox4x32_10((unsigned)jq, (unsigned)i, (unsigned)bh, a.d0, a.s0, a.s1, w);
}

__device__ __forceinline__ float ld_guard(const float* base, long row, int d, bool ok, long ld) { return ok ? base[row * ld + d] : 0.f; }

// RoPE of a run u[0 .. NS) = elements d0 .. d0+NS-1 (d0 even) of the row at position `pos`; ok: the row exists
template <int NS>
__device__ __forceinline__ void rope_run(const AttnArgs& a, float (&u)[NS], int pos, int d0, bool ok) {
    const int hh = a.hd >> 1;
#pragma unroll
    for (int t = 0; t < NS / 2; ++t) {
        const int pr = (d0 >> 1) + t;
        const bool in = ok && pr < hh;
        const float cs = in ? a.cos[(long)pos * hh + pr] : 1.f, sn = in ? a.sin[(long)pos * hh + pr] : 0.f;
        const float x0 = u[2 * t], x1 = u[2 * t + 1];
        u[2 * t] = x0 * cs - x1 * sn;
        u[2 * t + 1] = x0 * sn + x1 * cs;
    }
}

// RoPE of element d (= cc*16 + c: its pair partner d ^ 1 is lane ^ 1's) of the row at `pos`; every lane of the wave calls this
__device__ __forceinline__ float rope_col(const AttnArgs& a, float raw, int pos, int d, bool ok) {
    const float other = __shfl_xor(raw, 1, 64);
    const int hh = a.hd >> 1;
    const float cs = ok ? a.cos[(long)pos * hh + (d >> 1)] : 1.f, sn = ok ? a.sin[(long)pos * hh + (d >> 1)] : 0.f;
    return (d & 1) ? other * sn + raw * cs : raw * cs - other * sn;
}

// the transpose rotation of an accumulator fragment: reg r of acc[cc] is element cc*16 + 4g + r of the row at `pos` (pairs: r, r ^ 1)
template <int NC>
__device__ __forceinline__ void rope_back(const AttnArgs& a, f32x4 (&acc)[NC], int pos, int g) {
    const int hh = a.hd >> 1;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int pr = (cc * 16 + 4 * g) / 2 + t;
            const bool in = pr < hh;
            const float cs = in ? a.cos[(long)pos * hh + pr] : 1.f, sn = in ? a.sin[(long)pos * hh + pr] : 0.f;
            const float g0 = acc[cc][2 * t], g1 = acc[cc][2 * t + 1];
            acc[cc][2 * t] = g0 * cs + g1 * sn;
            acc[cc][2 * t + 1] = g1 * cs - g0 * sn;
        }
}

// wave-level tile order: work group t of the grid handles 4 consecutive 16-row tiles of one (b, h); `rev` maps the earliest
// dispatched groups to the LAST tiles (the longest causal rows) -- forward and dQ -- and the key passes keep t (key tile 0 sees
// every query)
__device__ __forceinline__ bool wave_tile(const AttnArgs& a, bool rev, int& tile, int& bh) {
    const int ngrp = (a.ntiles + 3) >> 2;
    const int t = blockIdx.x / a.nbh;
    bh = blockIdx.x - t * a.nbh;
    const int grp = rev ? ngrp - 1 - t : t;
    tile = grp * 4 + (threadIdx.x >> 6);
    return tile < a.ntiles;
}

template <int HDP, bool DROP, bool CAUSAL, bool ROPE>
__global__ __launch_bounds__(256) void attn_fwd_k(AttnArgs a) {
    constexpr int NS = HDP / 4, NC = HDP >= 16 ? HDP / 16 : 1;
    int qt, bh;
    if (!wave_tile(a, CAUSAL, qt, bh)) return;  // (no block-level barrier below: whole waves may leave)
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int b = bh / a.heads, h = bh - b * a.heads, L = a.L, hd = a.hd;
    const long row0 = (long)b * L;
    const float *qb = a.q + row0 * a.ld + h * hd, *kb = a.k + row0 * a.ld + h * hd, *vb = a.v + row0 * a.ld + h * hd;
    const int i0 = qt * 16, i = i0 + c;
    const float sl2 = a.scale * LOG2E;
    float qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = ld_guard(qb, i, g * NS + s, i < L && g * NS + s < hd, a.ld);
    if (ROPE) rope_run<NS>(a, qf, i, g * NS, i < L);
    f32x4 acc[NC];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) acc[cc] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    const int kend = CAUSAL ? qt + 1 : a.ntiles;
    for (int kt = 0; kt < kend; ++kt) {
        const int j0 = kt * 16, jr = j0 + c;
        f32x4 st = {0.f, 0.f, 0.f, 0.f};
        float kf[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) kf[s] = ld_guard(kb, jr, g * NS + s, jr < L && g * NS + s < hd, a.ld);
        if (ROPE) rope_run<NS>(a, kf, jr, g * NS, jr < L);
#pragma unroll
        for (int s = 0; s < NS; ++s) st = mfma4(kf[s], qf[s], st);
        float p[4], mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * g + r;
            p[r] = ((!CAUSAL || j <= i) && j < L) ? st[r] * sl2 : -INFINITY;
            mx = fmaxf(mx, p[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        // key 0 is in the first tile and visible to every lane (padded query rows included): mn is finite from there on, so a
        // padded last key tile (all -inf) gives p = 0
        const float mn = fmaxf(m, mx), alpha = exp2f(m - mn);
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[r] = exp2f(p[r] - mn);
            rs += p[r];
        }
        rs += __shfl_xor(rs, 16, 64);
        rs += __shfl_xor(rs, 32, 64);
        l = l * alpha + rs;
        m = mn;
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) acc[cc] *= alpha;
        if (DROP) {
            unsigned w[4];
            keep4(a, bh, i, (j0 >> 2) + g, w);
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] = w[r] < a.thr ? p[r] * a.inv_keep : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * g + r;
#pragma unroll
            for (int cc = 0; cc < NC; ++cc)
                acc[cc] = mfma4(ld_guard(vb, j, cc * 16 + c, j < L && cc * 16 + c < hd, a.ld), p[r], acc[cc]);
        }
    }
    if (i >= L) return;
    const float inv_l = 1.f / l;
    const int proj = a.heads * hd;
    float* ob = a.out + (row0 + i) * proj + h * a.oh;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = cc * 16 + 4 * g + r;
            if (d < hd) ob[(long)d * a.od] = acc[cc][r] * inv_l;
        }
    if (g == 0) a.lse_out[(long)bh * L + i] = (m + log2f(l)) * LN2;
}

// delta[bh][i] = sum_d dO[b][i][h*oh+d*od] * O[b][i][h*oh+d*od]  (D_i of the FlashAttention-2 backward; holds with dropout too)
__global__ __launch_bounds__(256) void attn_delta_k(const float* __restrict__ o, const float* __restrict__ dout, float* __restrict__ delta,
                                                    long rows, int heads, int L, int hd, int oh, int od) {
    const long n = rows * heads;  // (b, i, h)
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
        const long r = t / heads;
        const int h = (int)(t - r * heads);
        const float *ob = o + r * heads * hd + h * oh, *gb = dout + r * heads * hd + h * oh;
        float s = 0.f;
        for (int d = 0; d < hd; ++d) s += ob[(long)d * od] * gb[(long)d * od];
        const long b = r / L;
        delta[(b * heads + h) * L + (r - b * L)] = s;
    }
}

// dK, dV: one wave per 16-key tile, over the query tiles at and below the diagonal
template <int HDP, bool DROP, bool CAUSAL, bool ROPE>
__global__ __launch_bounds__(256) void attn_bwd_dkdv_k(AttnArgs a) {
    constexpr int NS = HDP / 4, NC = HDP >= 16 ? HDP / 16 : 1;
    int kt, bh;
    if (!wave_tile(a, false, kt, bh)) return;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int b = bh / a.heads, h = bh - b * a.heads, L = a.L, hd = a.hd, heads = a.heads;
    const long row0 = (long)b * L, ldo = (long)heads * hd;
    const float *qb = a.q + row0 * a.ld + h * hd, *kb = a.k + row0 * a.ld + h * hd, *vb = a.v + row0 * a.ld + h * hd;
    const float* gb = a.dout + row0 * ldo + h * a.oh;  // dO[i][d] at gb[i * ldo + d * od]
    const int od = a.od;
    const float *lseb = a.lse + (long)bh * L, *delb = a.delta + (long)bh * L;
    const int j0 = kt * 16, j = j0 + c;
    const float sl2 = a.scale * LOG2E;
    float kf[NS], vf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const bool ok = j < L && g * NS + s < hd;
        kf[s] = ld_guard(kb, j, g * NS + s, ok, a.ld);
        vf[s] = ld_guard(vb, j, g * NS + s, ok, a.ld);
    }
    if (ROPE) rope_run<NS>(a, kf, j, g * NS, j < L);
    f32x4 adk[NC], adv[NC];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) adk[cc] = adv[cc] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int qt = CAUSAL ? kt : 0; qt < a.ntiles; ++qt) {
        const int i0 = qt * 16, ir = i0 + c;
        f32x4 st = {0.f, 0.f, 0.f, 0.f}, dpt = {0.f, 0.f, 0.f, 0.f};
        float qr[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) qr[s] = ld_guard(qb, ir, g * NS + s, ir < L && g * NS + s < hd, a.ld);
        if (ROPE) rope_run<NS>(a, qr, ir, g * NS, ir < L);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int d = g * NS + s;
            const bool ok = ir < L && d < hd;
            st = mfma4(qr[s], kf[s], st);
            dpt = mfma4(ok ? gb[ir * ldo + (long)d * od] : 0.f, vf[s], dpt);
        }
        // keep bits of (query i0+4g+r, key j): lane (c, g) draws the Philox block of query i0+4g+(c&3), keys j0+4(c>>2) .. +3
        // -- the 4 x 4 patch its quad needs -- and the quad transposes it in 4 rotations: in rotation t lane k = c&3 takes from
        // quad lane (k+t)&3 the bit of word k, so each source sends one word (no lane reads a register index of its own choosing)
        unsigned kmask = 0xFu;
        if (DROP) {
            unsigned w[4];
            keep4(a, bh, i0 + 4 * g + (c & 3), (j0 >> 2) + (c >> 2), w);
            const int k = c & 3;
            kmask = 0u;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int sw = (k - t) & 3;  // the word this lane sends in rotation t
                const unsigned x = sw == 0 ? w[0] : sw == 1 ? w[1] : sw == 2 ? w[2] : w[3];
                const int src = (lane & ~3) | ((k + t) & 3);
                const int bit = __shfl((int)(x < a.thr), src, 64);
                kmask |= (unsigned)bit << ((k + t) & 3);
            }
        }
        float pk[4], ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * g + r;
            const bool ok = i < L && (CAUSAL ? j <= i : j < L);
            const float p = ok ? exp2f(st[r] * sl2 - lseb[i] * LOG2E) : 0.f;
            float dp = dpt[r], pd = p;
            if (DROP) {
                const bool kp = (kmask >> r) & 1u;
                dp = kp ? dp * a.inv_keep : 0.f;
                pd = kp ? p * a.inv_keep : 0.f;
            }
            pk[r] = pd;
            ds[r] = ok ? p * (dp - delb[i]) : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * g + r;
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                const int d = cc * 16 + c;
                const bool ok = i < L && d < hd;
                adv[cc] = mfma4(ok ? gb[i * ldo + (long)d * od] : 0.f, pk[r], adv[cc]);
                float qv = ld_guard(qb, i, d, ok, a.ld);
                if (ROPE) qv = rope_col(a, qv, i, d, ok);
                adk[cc] = mfma4(qv, ds[r], adk[cc]);
            }
        }
    }
    if (j >= L) return;
    if (ROPE) rope_back<NC>(a, adk, j, g);
    float *dkb = a.dk + (row0 + j) * a.ld + h * hd, *dvb = a.dv + (row0 + j) * a.ld + h * hd;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = cc * 16 + 4 * g + r;
            if (d < hd) {
                dkb[d] = adk[cc][r] * a.scale;
                dvb[d] = adv[cc][r];
            }
        }
}

// dQ: one wave per 16-query tile, over the key tiles at and left of the diagonal (the forward's orientation)
template <int HDP, bool DROP, bool CAUSAL, bool ROPE>
__global__ __launch_bounds__(256) void attn_bwd_dq_k(AttnArgs a) {
    constexpr int NS = HDP / 4, NC = HDP >= 16 ? HDP / 16 : 1;
    int qt, bh;
    if (!wave_tile(a, CAUSAL, qt, bh)) return;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int b = bh / a.heads, h = bh - b * a.heads, L = a.L, hd = a.hd, heads = a.heads;
    const long row0 = (long)b * L, ldo = (long)heads * hd;
    const float *qb = a.q + row0 * a.ld + h * hd, *kb = a.k + row0 * a.ld + h * hd, *vb = a.v + row0 * a.ld + h * hd;
    const float* gb = a.dout + row0 * ldo + h * a.oh;
    const int i0 = qt * 16, i = i0 + c;
    const float sl2 = a.scale * LOG2E;
    float qf[NS], gf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int d = g * NS + s;
        const bool ok = i < L && d < hd;
        qf[s] = ld_guard(qb, i, d, ok, a.ld);
        gf[s] = ok ? gb[i * ldo + (long)d * a.od] : 0.f;
    }
    if (ROPE) rope_run<NS>(a, qf, i, g * NS, i < L);
    const float lse2 = i < L ? a.lse[(long)bh * L + i] * LOG2E : 0.f, di = i < L ? a.delta[(long)bh * L + i] : 0.f;
    f32x4 acc[NC];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) acc[cc] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kend = CAUSAL ? qt + 1 : a.ntiles;
    for (int kt = 0; kt < kend; ++kt) {
        const int j0 = kt * 16, jr = j0 + c;
        f32x4 st = {0.f, 0.f, 0.f, 0.f}, dpt = {0.f, 0.f, 0.f, 0.f};
        float kf[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) kf[s] = ld_guard(kb, jr, g * NS + s, jr < L && g * NS + s < hd, a.ld);
        if (ROPE) rope_run<NS>(a, kf, jr, g * NS, jr < L);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int d = g * NS + s;
            const bool ok = jr < L && d < hd;
            st = mfma4(kf[s], qf[s], st);
            dpt = mfma4(ld_guard(vb, jr, d, ok, a.ld), gf[s], dpt);
        }
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (DROP) keep4(a, bh, i, (j0 >> 2) + g, w);
        float ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * g + r;
            const bool ok = i < L && (CAUSAL ? j <= i : j < L);
            const float p = ok ? exp2f(st[r] * sl2 - lse2) : 0.f;
            float dp = dpt[r];
            if (DROP) dp = w[r] < a.thr ? dp * a.inv_keep : 0.f;
            ds[r] = p * (dp - di);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * g + r;
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
                const int d = cc * 16 + c;
                const bool okk = j < L && d < hd;
                float kv = ld_guard(kb, j, d, okk, a.ld);
                if (ROPE) kv = rope_col(a, kv, j, d, okk);
                acc[cc] = mfma4(kv, ds[r], acc[cc]);
            }
        }
    }
    if (i >= L) return;
    if (ROPE) rope_back<NC>(a, acc, i, g);
    float* dqb = a.dq + (row0 + i) * a.ld + h * hd;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = cc * 16 + 4 * g + r;
            if (d < hd) dqb[d] = acc[cc][r] * a.scale;
        }
}

// keep[bh][i][j] in {0, 1} for every (i, j) < L (test / measurement hook; the kernels above never store the mask)
__global__ __launch_bounds__(256) void attn_mask_k(AttnArgs a, uint8_t* __restrict__ keep, long n4) {
    const int L = a.L, LQ = (L + 3) >> 2;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n4; t += (long)gridDim.x * blockDim.x) {
        const long row = t / LQ;  // bh * L + i
        const int jq = (int)(t - row * LQ);
        const int bh = (int)(row / L), i = (int)(row - (long)bh * L);
        unsigned w[4];
        keep4(a, bh, i, jq, w);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (jq * 4 + r < L) keep[row * L + jq * 4 + r] = (!a.drop || w[r] < a.thr) ? 1 : 0;
    }
}

// ---- bf16-operand instances (movae_set_compute_dtype(MOVAE_DTYPE_BF16); see the header) --------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

constexpr int BF_STEP = 32;  // keys (queries in dK / dV) per loop step: one 32-deep MFMA step of the second product
constexpr int BF_LDT = 36;   // halfs per row of a transposed image: 32 positions + 4 of padding (72-byte rows)

__device__ __forceinline__ f32x4 mfma32(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// A tensor as the staging code sees it: element (row, d) of this (b, h) at p[row * ld + d * ds]
struct BfSrc {
    const float* p;
    long ld;
    int ds;
    bool v4;  // every aligned group of 4 consecutive d of a row is one aligned 16-byte run (block-uniform)
};
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ BfSrc bf_src(const float* p, long ld, int ds, int hd) {
    return BfSrc{p, ld, ds, ds == 1 && (ld & 3) == 0 && (hd & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0};
}

// Row image R[32][HDP + 8] (bf16, d contiguous): rows r0 .. r0+31 of `src`, rotated if ROPE, zero beyond L / hd.  Item = (row,
// 4 consecutive d); a thread holds HDP / 32 of them between its global loads and its LDS stores.
template <int HDP, bool ROPE>
__device__ __forceinline__ void row_load(const AttnArgs& a, const BfSrc& src, int r0, f32x4 (&v)[HDP / 32]) {
#pragma unroll
    for (int n = 0; n < HDP / 32; ++n) {
        const int it = threadIdx.x + 256 * n, row = r0 + it / (HDP / 4), d0 = (it % (HDP / 4)) * 4;
        float u[4];
        if (src.v4) {
            const f32x4 t = (row < a.L && d0 < a.hd) ? *reinterpret_cast<const f32x4*>(src.p + row * src.ld + d0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] = t[e];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] = (row < a.L && d0 + e < a.hd) ? src.p[row * src.ld + (long)(d0 + e) * src.ds] : 0.f;
        }
        if (ROPE) rope_run<4>(a, u, row, d0, row < a.L);
        v[n] = f32x4{u[0], u[1], u[2], u[3]};
    }
}
template <int HDP>
__device__ __forceinline__ void row_store(__bf16* __restrict__ R, const f32x4 (&v)[HDP / 32]) {
#pragma unroll
    for (int n = 0; n < HDP / 32; ++n) {
        const int it = threadIdx.x + 256 * n;
        *reinterpret_cast<bf16x4*>(R + (it / (HDP / 4)) * (HDP + 8) + (it % (HDP / 4)) * 4) = __builtin_convertvector(v[n], bf16x4);
    }
}

// Transposed image T[NC * 16][BF_LDT] (bf16, position contiguous) of the same rows.  Item = (4 consecutive rows, one RoPE pair of
// d): 64 * NC items, one for each of the first 64 * NC threads; u[2e + x] = element 2 * pair + x of row 4 * quad + e.
template <int NC, bool ROPE>
__device__ __forceinline__ void tr_load(const AttnArgs& a, const BfSrc& src, int r0, float (&u)[8]) {
    const int it = threadIdx.x;
    if (it >= 64 * NC) return;
    const int pr = it % (NC * 8), kq = it / (NC * 8), hh = a.hd >> 1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int row = r0 + 4 * kq + e;
        float x0, x1;
        if (src.v4) {
            const f32x2 t = (row < a.L && 2 * pr < a.hd) ? *reinterpret_cast<const f32x2*>(src.p + row * src.ld + 2 * pr) : f32x2{0.f, 0.f};
            x0 = t[0], x1 = t[1];
        } else {
            x0 = (row < a.L && 2 * pr < a.hd) ? src.p[row * src.ld + (long)(2 * pr) * src.ds] : 0.f;
            x1 = (row < a.L && 2 * pr + 1 < a.hd) ? src.p[row * src.ld + (long)(2 * pr + 1) * src.ds] : 0.f;
        }
        if (ROPE && row < a.L && pr < hh) {
            const float cs = a.cos[(long)row * hh + pr], sn = a.sin[(long)row * hh + pr], y0 = x0;
            x0 = y0 * cs - x1 * sn;
            x1 = y0 * sn + x1 * cs;
        }
        u[2 * e] = x0, u[2 * e + 1] = x1;
    }
}
template <int NC>
__device__ __forceinline__ void tr_store(__bf16* __restrict__ T, const float (&u)[8]) {
    const int it = threadIdx.x;
    if (it >= 64 * NC) return;
    const int pr = it % (NC * 8), kq = it / (NC * 8);
    *reinterpret_cast<bf16x4*>(T + (2 * pr) * BF_LDT + 4 * kq) = __builtin_convertvector((f32x4{u[0], u[2], u[4], u[6]}), bf16x4);
    *reinterpret_cast<bf16x4*>(T + (2 * pr + 1) * BF_LDT + 4 * kq) = __builtin_convertvector((f32x4{u[1], u[3], u[5], u[7]}), bf16x4);
}

// The wave's own 16 rows as the B operand of the first product: lane (c, g) holds elements 32 ks + 8 g .. + 7 of row `row`
template <int HDP, bool ROPE>
__device__ __forceinline__ void own_frag(const AttnArgs& a, const BfSrc& src, int row, int g, bf16x8 (&f)[HDP / 32]) {
#pragma unroll
    for (int ks = 0; ks < HDP / 32; ++ks) {
        const int d0 = 32 * ks + 8 * g;
        float u[8];
        if (src.v4) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const f32x4 t = (row < a.L && d0 + 4 * q < a.hd) ? *reinterpret_cast<const f32x4*>(src.p + row * src.ld + d0 + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) u[4 * q + e] = t[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) u[e] = (row < a.L && d0 + e < a.hd) ? src.p[row * src.ld + (long)(d0 + e) * src.ds] : 0.f;
        }
        if (ROPE) rope_run<8>(a, u, row, d0, row < a.L);
        f[ks] = __builtin_convertvector((f32x8{u[0], u[1], u[2], u[3], u[4], u[5], u[6], u[7]}), bf16x8);
    }
}

// first product of a pair: rows 16 s + c of a row image against the wave's own fragment
template <int HDP>
__device__ __forceinline__ f32x4 mma_rows(const __bf16* __restrict__ R, int s, int c, int g, const bf16x8 (&own)[HDP / 32]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < HDP / 32; ++ks)
        acc = mfma32(*reinterpret_cast<const bf16x8*>(R + (16 * s + c) * (HDP + 8) + 32 * ks + 8 * g), own[ks], acc);
    return acc;
}

// second product of a pair: acc[cc] (row d = cc * 16 + 4 g + r, column = the wave's row c) += T[d][pos] * x[pos], x the first
// product's two accumulators.  k slot (g, e) of the 32-deep step is position 16 (e >> 2) + 4 g + (e & 3) on BOTH operands: x packs
// its registers in that order and T is read as the two 4-position runs at 4 g and 16 + 4 g.
template <int NC>
__device__ __forceinline__ void mma_cols(const __bf16* __restrict__ T, int c, int g, const float (&x0)[4], const float (&x1)[4], f32x4 (&acc)[NC]) {
    const bf16x8 xb = __builtin_convertvector((f32x8{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]}), bf16x8);
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
        const __bf16* t = T + (cc * 16 + c) * BF_LDT + 4 * g;
        const bf16x4 lo = *reinterpret_cast<const bf16x4*>(t), hi = *reinterpret_cast<const bf16x4*>(t + 16);
        acc[cc] = mfma32(__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7), xb, acc[cc]);
    }
}

// block-level tile order: work group t handles 4 consecutive 16-row tiles of one (b, h), one per wave (wave_tile's order)
__device__ __forceinline__ void block_tile(const AttnArgs& a, bool rev, int& grp, int& bh) {
    const int ngrp = (a.ntiles + 3) >> 2;
    const int t = blockIdx.x / a.nbh;
    bh = blockIdx.x - t * a.nbh;
    grp = rev ? ngrp - 1 - t : t;
}

// NC: 16-wide chunks of the head dim that exist (1, 2 or 4); the reduction over d is padded to HDP = 32 or 64
template <int NC, bool DROP, bool CAUSAL, bool ROPE>
__global__ __launch_bounds__(256) void attn_fwd_bf_k(AttnArgs a) {
    constexpr int HDP = NC <= 2 ? 32 : 64, KS = HDP / 32;
    __shared__ __attribute__((aligned(16))) __bf16 Ks[BF_STEP * (HDP + 8)];
    __shared__ __attribute__((aligned(16))) __bf16 Vt[NC * 16 * BF_LDT];
    int grp, bh;
    block_tile(a, CAUSAL, grp, bh);
    const int qt = grp * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int b = bh / a.heads, h = bh - b * a.heads, L = a.L, hd = a.hd;
    const long row0 = (long)b * L;
    const BfSrc qs = bf_src(a.q + row0 * a.ld + h * hd, a.ld, 1, hd), ks = bf_src(a.k + row0 * a.ld + h * hd, a.ld, 1, hd),
                vs = bf_src(a.v + row0 * a.ld + h * hd, a.ld, 1, hd);
    const int i0 = qt * 16, i = i0 + c;
    const float sl2 = a.scale * LOG2E;
    bf16x8 qf[KS];
    own_frag<HDP, ROPE>(a, qs, i, g, qf);
    f32x4 acc[NC];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) acc[cc] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    const int kend = CAUSAL ? min(L, (grp * 4 + 4) * 16) : L;  // keys the block's last query tile sees
    const int nsteps = (kend + BF_STEP - 1) / BF_STEP;
    f32x4 kreg[KS];
    float vreg[8];
    row_load<HDP, ROPE>(a, ks, 0, kreg);
    tr_load<NC, false>(a, vs, 0, vreg);
    for (int step = 0; step < nsteps; ++step) {
        __syncthreads();  // every wave is done with the previous tile
        row_store<HDP>(Ks, kreg);
        tr_store<NC>(Vt, vreg);
        __syncthreads();
        if (step + 1 < nsteps) {
            row_load<HDP, ROPE>(a, ks, (step + 1) * BF_STEP, kreg);
            tr_load<NC, false>(a, vs, (step + 1) * BF_STEP, vreg);
        }
        const int j0 = step * BF_STEP;
        if (qt >= a.ntiles || (CAUSAL && j0 > i0 + 15)) continue;  // (wave-uniform; the barriers are above)
        float p[2][4], mx = -INFINITY;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const f32x4 st = mma_rows<HDP>(Ks, s, c, g, qf);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + 16 * s + 4 * g + r;
                p[s][r] = ((!CAUSAL || j <= i) && j < L) ? st[r] * sl2 : -INFINITY;
                mx = fmaxf(mx, p[s][r]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        // key 0 is in the first step and visible to every lane (padded query rows included): mn is finite from there on
        const float mn = fmaxf(m, mx), alpha = exp2f(m - mn);
        float rs = 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[s][r] = exp2f(p[s][r] - mn);
                rs += p[s][r];  // the row sum takes the unrounded probabilities
            }
        rs += __shfl_xor(rs, 16, 64);
        rs += __shfl_xor(rs, 32, 64);
        l = l * alpha + rs;
        m = mn;
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) acc[cc] *= alpha;
        if (DROP) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                unsigned w[4];
                keep4(a, bh, i, (j0 >> 2) + 4 * s + g, w);
#pragma unroll
                for (int r = 0; r < 4; ++r) p[s][r] = w[r] < a.thr ? p[s][r] * a.inv_keep : 0.f;
            }
        }
        mma_cols<NC>(Vt, c, g, p[0], p[1], acc);
    }
    if (i >= L) return;
    const float inv_l = 1.f / l;
    const int proj = a.heads * hd;
    float* ob = a.out + (row0 + i) * proj + h * a.oh;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = cc * 16 + 4 * g + r;
            if (d < hd) ob[(long)d * a.od] = acc[cc][r] * inv_l;
        }
    if (g == 0) a.lse_out[(long)bh * L + i] = (m + log2f(l)) * LN2;
}

// keep bits of (query iq0 + r, key j0 + c), r = 0 .. 3, as bits of the result: attn_bwd_dkdv_k's quad transpose
__device__ __forceinline__ unsigned keep_quad(const AttnArgs& a, int bh, int iq0, int j0, int lane) {
    const int c = lane & 15, k = c & 3;
    unsigned w[4];
    keep4(a, bh, iq0 + k, (j0 >> 2) + (c >> 2), w);
    unsigned kmask = 0u;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int sw = (k - t) & 3;
        const unsigned x = sw == 0 ? w[0] : sw == 1 ? w[1] : sw == 2 ? w[2] : w[3];
        const int src = (lane & ~3) | ((k + t) & 3);
        const int bit = __shfl((int)(x < a.thr), src, 64);
        kmask |= (unsigned)bit << ((k + t) & 3);
    }
    return kmask;
}

template <int NC, bool DROP, bool CAUSAL, bool ROPE>
__global__ __launch_bounds__(256) void attn_bwd_dkdv_bf_k(AttnArgs a) {
    constexpr int HDP = NC <= 2 ? 32 : 64, KS = HDP / 32;
    __shared__ __attribute__((aligned(16))) __bf16 Qs[BF_STEP * (HDP + 8)];
    __shared__ __attribute__((aligned(16))) __bf16 Gs[BF_STEP * (HDP + 8)];
    __shared__ __attribute__((aligned(16))) __bf16 Qt[NC * 16 * BF_LDT];
    __shared__ __attribute__((aligned(16))) __bf16 Gt[NC * 16 * BF_LDT];
    int grp, bh;
    block_tile(a, false, grp, bh);
    const int kt = grp * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int b = bh / a.heads, h = bh - b * a.heads, L = a.L, hd = a.hd, heads = a.heads;
    const long row0 = (long)b * L;
    const BfSrc qs = bf_src(a.q + row0 * a.ld + h * hd, a.ld, 1, hd), ks = bf_src(a.k + row0 * a.ld + h * hd, a.ld, 1, hd),
                vs = bf_src(a.v + row0 * a.ld + h * hd, a.ld, 1, hd);
    const BfSrc gs = bf_src(a.dout + row0 * heads * hd + h * a.oh, (long)heads * hd, a.od, hd);
    const float *lseb = a.lse + (long)bh * L, *delb = a.delta + (long)bh * L;
    const int j0 = kt * 16, j = j0 + c;
    const float sl2 = a.scale * LOG2E;
    bf16x8 kf[KS], vf[KS];
    own_frag<HDP, ROPE>(a, ks, j, g, kf);
    own_frag<HDP, false>(a, vs, j, g, vf);
    f32x4 adk[NC], adv[NC];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) adk[cc] = adv[cc] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ibeg = CAUSAL ? grp * 64 : 0;  // the block's first key tile starts here: no earlier query sees any of its keys
    const int nsteps = (L - ibeg + BF_STEP - 1) / BF_STEP;
    f32x4 qreg[KS], greg[KS];
    float qtr[8], gtr[8];
    row_load<HDP, ROPE>(a, qs, ibeg, qreg);
    row_load<HDP, false>(a, gs, ibeg, greg);
    tr_load<NC, ROPE>(a, qs, ibeg, qtr);
    tr_load<NC, false>(a, gs, ibeg, gtr);
    for (int step = 0; step < nsteps; ++step) {
        __syncthreads();
        row_store<HDP>(Qs, qreg);
        row_store<HDP>(Gs, greg);
        tr_store<NC>(Qt, qtr);
        tr_store<NC>(Gt, gtr);
        __syncthreads();
        const int i0 = ibeg + step * BF_STEP;
        if (step + 1 < nsteps) {
            row_load<HDP, ROPE>(a, qs, i0 + BF_STEP, qreg);
            row_load<HDP, false>(a, gs, i0 + BF_STEP, greg);
            tr_load<NC, ROPE>(a, qs, i0 + BF_STEP, qtr);
            tr_load<NC, false>(a, gs, i0 + BF_STEP, gtr);
        }
        if (kt >= a.ntiles || (CAUSAL && i0 + BF_STEP - 1 < j0)) continue;  // (wave-uniform)
        float pk[2][4], ds[2][4];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const f32x4 st = mma_rows<HDP>(Qs, s, c, g, kf), dpt = mma_rows<HDP>(Gs, s, c, g, vf);
            unsigned kmask = 0xFu;
            if (DROP) kmask = keep_quad(a, bh, i0 + 16 * s + 4 * g, j0, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + 16 * s + 4 * g + r;
                const bool ok = i < L && (CAUSAL ? j <= i : j < L);
                const float p = ok ? exp2f(st[r] * sl2 - lseb[i] * LOG2E) : 0.f;
                float dp = dpt[r], pd = p;
                if (DROP) {
                    const bool kp = (kmask >> r) & 1u;
                    dp = kp ? dp * a.inv_keep : 0.f;
                    pd = kp ? p * a.inv_keep : 0.f;
                }
                pk[s][r] = pd;
                ds[s][r] = ok ? p * (dp - delb[i]) * a.scale : 0.f;
            }
        }
        mma_cols<NC>(Gt, c, g, pk[0], pk[1], adv);
        mma_cols<NC>(Qt, c, g, ds[0], ds[1], adk);
    }
    if (kt >= a.ntiles || j >= L) return;
    if (ROPE) rope_back<NC>(a, adk, j, g);
    float *dkb = a.dk + (row0 + j) * a.ld + h * hd, *dvb = a.dv + (row0 + j) * a.ld + h * hd;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = cc * 16 + 4 * g + r;
            if (d < hd) {
                dkb[d] = adk[cc][r];  // (1 / sqrt(hd) is inside dS)
                dvb[d] = adv[cc][r];
            }
        }
}

template <int NC, bool DROP, bool CAUSAL, bool ROPE>
__global__ __launch_bounds__(256) void attn_bwd_dq_bf_k(AttnArgs a) {
    constexpr int HDP = NC <= 2 ? 32 : 64, KS = HDP / 32;
    __shared__ __attribute__((aligned(16))) __bf16 Ks[BF_STEP * (HDP + 8)];
    __shared__ __attribute__((aligned(16))) __bf16 Vs[BF_STEP * (HDP + 8)];
    __shared__ __attribute__((aligned(16))) __bf16 Kt[NC * 16 * BF_LDT];
    int grp, bh;
    block_tile(a, CAUSAL, grp, bh);
    const int qt = grp * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int b = bh / a.heads, h = bh - b * a.heads, L = a.L, hd = a.hd, heads = a.heads;
    const long row0 = (long)b * L;
    const BfSrc qs = bf_src(a.q + row0 * a.ld + h * hd, a.ld, 1, hd), ks = bf_src(a.k + row0 * a.ld + h * hd, a.ld, 1, hd),
                vs = bf_src(a.v + row0 * a.ld + h * hd, a.ld, 1, hd);
    const BfSrc gs = bf_src(a.dout + row0 * heads * hd + h * a.oh, (long)heads * hd, a.od, hd);
    const int i0 = qt * 16, i = i0 + c;
    const float sl2 = a.scale * LOG2E;
    bf16x8 qf[KS], gf[KS];
    own_frag<HDP, ROPE>(a, qs, i, g, qf);
    own_frag<HDP, false>(a, gs, i, g, gf);
    const float lse2 = i < L ? a.lse[(long)bh * L + i] * LOG2E : 0.f, di = i < L ? a.delta[(long)bh * L + i] : 0.f;
    f32x4 acc[NC];
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) acc[cc] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kend = CAUSAL ? min(L, (grp * 4 + 4) * 16) : L;
    const int nsteps = (kend + BF_STEP - 1) / BF_STEP;
    f32x4 kreg[KS], vreg[KS];
    float ktr[8];
    row_load<HDP, ROPE>(a, ks, 0, kreg);
    row_load<HDP, false>(a, vs, 0, vreg);
    tr_load<NC, ROPE>(a, ks, 0, ktr);
    for (int step = 0; step < nsteps; ++step) {
        __syncthreads();
        row_store<HDP>(Ks, kreg);
        row_store<HDP>(Vs, vreg);
        tr_store<NC>(Kt, ktr);
        __syncthreads();
        const int j0 = step * BF_STEP;
        if (step + 1 < nsteps) {
            row_load<HDP, ROPE>(a, ks, j0 + BF_STEP, kreg);
            row_load<HDP, false>(a, vs, j0 + BF_STEP, vreg);
            tr_load<NC, ROPE>(a, ks, j0 + BF_STEP, ktr);
        }
        if (qt >= a.ntiles || (CAUSAL && j0 > i0 + 15)) continue;  // (wave-uniform)
        float ds[2][4];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const f32x4 st = mma_rows<HDP>(Ks, s, c, g, qf), dpt = mma_rows<HDP>(Vs, s, c, g, gf);
            unsigned w[4] = {0u, 0u, 0u, 0u};
            if (DROP) keep4(a, bh, i, (j0 >> 2) + 4 * s + g, w);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + 16 * s + 4 * g + r;
                const bool ok = i < L && (CAUSAL ? j <= i : j < L);
                const float p = ok ? exp2f(st[r] * sl2 - lse2) : 0.f;
                float dp = dpt[r];
                if (DROP) dp = w[r] < a.thr ? dp * a.inv_keep : 0.f;
                ds[s][r] = p * (dp - di) * a.scale;
            }
        }
        mma_cols<NC>(Kt, c, g, ds[0], ds[1], acc);
    }
    if (i >= L) return;
    if (ROPE) rope_back<NC>(a, acc, i, g);
    float* dqb = a.dq + (row0 + i) * a.ld + h * hd;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = cc * 16 + 4 * g + r;
            if (d < hd) dqb[d] = acc[cc][r];  // (1 / sqrt(hd) is inside dS)
        }
}

int hdp_of(int hd) { return hd <= 8 ? 8 : hd <= 16 ? 16 : hd <= 32 ? 32 : 64; }

// common argument checks and the per-call constants; rc != MOVAE_OK: error already set
int setup(AttnArgs& a, const char* what, long ld, int B, int heads, int L, int hd, float p, unsigned long long seed, unsigned long long draw) {
    MOVAE_CHECK_ARG(B > 0 && heads > 0 && L > 0 && hd > 0, "%s: bad sizes B=%d heads=%d L=%d head_dim=%d", what, B, heads, L, hd);
    MOVAE_CHECK_ARG(hd <= 64, "%s: head_dim %d exceeds the supported maximum of 64", what, hd);
    MOVAE_CHECK_ARG(ld >= (long)heads * hd, "%s: row stride %ld < heads * head_dim", what, ld);
    MOVAE_CHECK_ARG(p >= 0.f && p < 1.f, "%s: dropout p must be in [0, 1), got %g", what, (double)p);
    MOVAE_CHECK_ARG((long)B * heads <= (1L << 30) && L <= (1 << 28), "%s: sizes out of range", what);
    a = AttnArgs{};
    a.ld = ld;
    a.oh = 1, a.od = heads;  // PixelSNAIL's channel order d * heads + h
    a.heads = heads, a.L = L, a.hd = hd;
    a.ntiles = (L + 15) / 16;
    a.nbh = B * heads;
    a.scale = 1.f / sqrtf((float)hd);
    const double t = (1.0 - (double)p) * 4294967296.0;
    a.thr = p > 0.f ? (unsigned)(t >= 4294967295.0 ? 4294967295.0 : t) : 0xFFFFFFFFu;
    a.drop = p > 0.f;
    a.inv_keep = p > 0.f ? (float)(1.0 / (1.0 - (double)p)) : 1.f;
    a.s0 = (unsigned)seed, a.s1 = (unsigned)(seed >> 32) ^ (unsigned)(draw >> 32), a.d0 = (unsigned)draw;
    return MOVAE_OK;
}

dim3 tile_grid(const AttnArgs& a) { return dim3((unsigned)(((a.ntiles + 3) / 4) * a.nbh)); }

// one template instance per padded head dim (8 / 16 / 32 / 64) and dropout on / off
#define ATTN_LAUNCH(KERNEL, a, drop, stream)                                                              \
    do {                                                                                                  \
        const dim3 grid_ = tile_grid(a);                                                                  \
        const int hdp_ = hdp_of((a).hd);                                                                  \
        if (hdp_ == 8) {                                                                                  \
            if (drop) hipLaunchKernelGGL((KERNEL<8, true, true, false>), grid_, dim3(256), 0, stream, a);  \
            else hipLaunchKernelGGL((KERNEL<8, false, true, false>), grid_, dim3(256), 0, stream, a);      \
        } else if (hdp_ == 16) {                                                                          \
            if (drop) hipLaunchKernelGGL((KERNEL<16, true, true, false>), grid_, dim3(256), 0, stream, a);             \
            else hipLaunchKernelGGL((KERNEL<16, false, true, false>), grid_, dim3(256), 0, stream, a);                 \
        } else if (hdp_ == 32) {                                                                          \
            if (drop) hipLaunchKernelGGL((KERNEL<32, true, true, false>), grid_, dim3(256), 0, stream, a);             \
            else hipLaunchKernelGGL((KERNEL<32, false, true, false>), grid_, dim3(256), 0, stream, a);                 \
        } else {                                                                                          \
            if (drop) hipLaunchKernelGGL((KERNEL<64, true, true, false>), grid_, dim3(256), 0, stream, a);             \
            else hipLaunchKernelGGL((KERNEL<64, false, true, false>), grid_, dim3(256), 0, stream, a);                 \
        }                                                                                                 \
    } while (0)

// the bidirectional instances: no dropout, RoPE on / off
#define ATTN_LAUNCH_BIDIR(KERNEL, a, rope, stream)                                                                 \
    do {                                                                                                           \
        const dim3 grid_ = tile_grid(a);                                                                           \
        const int hdp_ = hdp_of((a).hd);                                                                           \
        if (hdp_ == 8) {                                                                                           \
            if (rope) hipLaunchKernelGGL((KERNEL<8, false, false, true>), grid_, dim3(256), 0, stream, a);         \
            else hipLaunchKernelGGL((KERNEL<8, false, false, false>), grid_, dim3(256), 0, stream, a);             \
        } else if (hdp_ == 16) {                                                                                   \
            if (rope) hipLaunchKernelGGL((KERNEL<16, false, false, true>), grid_, dim3(256), 0, stream, a);        \
            else hipLaunchKernelGGL((KERNEL<16, false, false, false>), grid_, dim3(256), 0, stream, a);            \
        } else if (hdp_ == 32) {                                                                                   \
            if (rope) hipLaunchKernelGGL((KERNEL<32, false, false, true>), grid_, dim3(256), 0, stream, a);        \
            else hipLaunchKernelGGL((KERNEL<32, false, false, false>), grid_, dim3(256), 0, stream, a);            \
        } else {                                                                                                   \
            if (rope) hipLaunchKernelGGL((KERNEL<64, false, false, true>), grid_, dim3(256), 0, stream, a);        \
            else hipLaunchKernelGGL((KERNEL<64, false, false, false>), grid_, dim3(256), 0, stream, a);            \
        }                                                                                                          \
    } while (0)

// the bf16-operand instances: one per count of 16-wide head-dim chunks (1 / 2 / 4) and, causal: dropout on / off; bidirectional:
// RoPE on / off (`flag`)
#define ATTN_BF_ONE(KERNEL, NC, a, causal, flag, stream)                                                                   \
    do {                                                                                                                   \
        if (causal) {                                                                                                      \
            if (flag) hipLaunchKernelGGL((KERNEL<NC, true, true, false>), grid_, dim3(256), 0, stream, a);                 \
            else hipLaunchKernelGGL((KERNEL<NC, false, true, false>), grid_, dim3(256), 0, stream, a);                     \
        } else {                                                                                                           \
            if (flag) hipLaunchKernelGGL((KERNEL<NC, false, false, true>), grid_, dim3(256), 0, stream, a);                \
            else hipLaunchKernelGGL((KERNEL<NC, false, false, false>), grid_, dim3(256), 0, stream, a);                    \
        }                                                                                                                  \
    } while (0)
#define ATTN_LAUNCH_BF(KERNEL, a, causal, flag, stream)                    \
    do {                                                                   \
        const dim3 grid_ = tile_grid(a);                                   \
        if ((a).hd <= 16) ATTN_BF_ONE(KERNEL, 1, a, causal, flag, stream); \
        else if ((a).hd <= 32) ATTN_BF_ONE(KERNEL, 2, a, causal, flag, stream); \
        else ATTN_BF_ONE(KERNEL, 4, a, causal, flag, stream);              \
    } while (0)

// argument checks of the bidirectional entry points beyond setup()'s
int setup_bidir(AttnArgs& a, const char* what, long ld, const float* cs, const float* sn, int B, int heads, int L, int hd, float p) {
    MOVAE_CHECK_ARG(p == 0.f, "%s: attention dropout is not supported (p must be 0, got %g)", what, (double)p);
    MOVAE_CHECK_ARG((cs == nullptr) == (sn == nullptr), "%s: give both RoPE tables (cos and sin) or neither", what);
    MOVAE_CHECK_ARG(!cs || (hd > 0 && hd % 2 == 0), "%s: RoPE needs an even head_dim, got %d", what, hd);
    const int rc = setup(a, what, ld, B, heads, L, hd, 0.f, 0ull, 0ull);
    if (rc != MOVAE_OK) return rc;
    a.cos = cs, a.sin = sn;
    a.oh = hd, a.od = 1;  // head-major: (attn @ v).transpose(1, 2).reshape(B, N, C)
    return MOVAE_OK;
}

}  // namespace

extern "C" {

int movae_causal_attn_fwd(const float* q, const float* k, const float* v, long ld, float* out, float* lse, int B, int heads, int L,
                          int hd, float p, unsigned long long seed, unsigned long long draw, movae_stream_t stream) {
    MOVAE_CHECK_ARG(q && k && v && out && lse, "movae_causal_attn_fwd: null pointer");
    AttnArgs a;
    const int rc = setup(a, "movae_causal_attn_fwd", ld, B, heads, L, hd, p, seed, draw);
    if (rc != MOVAE_OK) return rc;
    a.q = q, a.k = k, a.v = v, a.out = out, a.lse_out = lse;
    const bool drop = p > 0.f;
    if (g_movae_compute_bf16) ATTN_LAUNCH_BF(attn_fwd_bf_k, a, true, drop, (hipStream_t)stream);
    else ATTN_LAUNCH(attn_fwd_k, a, drop, (hipStream_t)stream);
    MOVAE_CHECK_LAUNCH("causal_attn_fwd");
    return MOVAE_OK;
}

size_t movae_causal_attn_ws_bytes(int B, int heads, int L) {
    return MOVAE_WS_HEADER_BYTES + (size_t)B * heads * L * sizeof(float);
}

int movae_causal_attn_bwd(const float* q, const float* k, const float* v, long ld, const float* out, const float* dout, const float* lse,
                          float* dq, float* dk, float* dv, int B, int heads, int L, int hd, float p, unsigned long long seed,
                          unsigned long long draw, void* ws, size_t ws_bytes, movae_stream_t stream) {
    MOVAE_WS_SCRATCH(ws, ws_bytes);
    MOVAE_CHECK_ARG(q && k && v && out && dout && lse && dq && dk && dv, "movae_causal_attn_bwd: null pointer");
    AttnArgs a;
    const int rc = setup(a, "movae_causal_attn_bwd", ld, B, heads, L, hd, p, seed, draw);
    if (rc != MOVAE_OK) return rc;
    MOVAE_CHECK_ARG(ws && ws_bytes >= (size_t)B * heads * L * sizeof(float), "movae_causal_attn_bwd: workspace too small");
    float* delta = static_cast<float*>(ws);
    const long rows = (long)B * L;
    const long n = rows * heads;
    long g = (n + 255) / 256;
    g = g > 8192 ? 8192 : g;
    hipLaunchKernelGGL(attn_delta_k, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, out, dout, delta, rows, heads, L, hd,
                       a.oh, a.od);
    MOVAE_CHECK_LAUNCH("causal_attn_delta");
    a.q = q, a.k = k, a.v = v, a.dout = dout, a.lse = lse, a.delta = delta, a.dq = dq, a.dk = dk, a.dv = dv;
    const bool drop = p > 0.f;
    if (g_movae_compute_bf16) ATTN_LAUNCH_BF(attn_bwd_dkdv_bf_k, a, true, drop, (hipStream_t)stream);
    else ATTN_LAUNCH(attn_bwd_dkdv_k, a, drop, (hipStream_t)stream);
    MOVAE_CHECK_LAUNCH("causal_attn_bwd_dkdv");
    if (g_movae_compute_bf16) ATTN_LAUNCH_BF(attn_bwd_dq_bf_k, a, true, drop, (hipStream_t)stream);
    else ATTN_LAUNCH(attn_bwd_dq_k, a, drop, (hipStream_t)stream);
    MOVAE_CHECK_LAUNCH("causal_attn_bwd_dq");
    return MOVAE_OK;
}

int movae_attn_fwd(const float* q, const float* k, const float* v, long ld, const float* rope_cos, const float* rope_sin, float* out,
                   float* lse, int B, int heads, int L, int hd, float p, movae_stream_t stream) {
    MOVAE_CHECK_ARG(q && k && v && out && lse, "movae_attn_fwd: null pointer");
    AttnArgs a;
    const int rc = setup_bidir(a, "movae_attn_fwd", ld, rope_cos, rope_sin, B, heads, L, hd, p);
    if (rc != MOVAE_OK) return rc;
    a.q = q, a.k = k, a.v = v, a.out = out, a.lse_out = lse;
    const bool rope = rope_cos != nullptr;
    if (g_movae_compute_bf16) ATTN_LAUNCH_BF(attn_fwd_bf_k, a, false, rope, (hipStream_t)stream);
    else ATTN_LAUNCH_BIDIR(attn_fwd_k, a, rope, (hipStream_t)stream);
    MOVAE_CHECK_LAUNCH("attn_fwd");
    return MOVAE_OK;
}

size_t movae_attn_ws_bytes(int B, int heads, int L) { return movae_causal_attn_ws_bytes(B, heads, L); }

int movae_attn_bwd(const float* q, const float* k, const float* v, long ld, const float* rope_cos, const float* rope_sin, const float* out,
                   const float* dout, const float* lse, float* dq, float* dk, float* dv, int B, int heads, int L, int hd, float p, void* ws,
                   size_t ws_bytes, movae_stream_t stream) {
    MOVAE_WS_SCRATCH(ws, ws_bytes);
    MOVAE_CHECK_ARG(q && k && v && out && dout && lse && dq && dk && dv, "movae_attn_bwd: null pointer");
    AttnArgs a;
    const int rc = setup_bidir(a, "movae_attn_bwd", ld, rope_cos, rope_sin, B, heads, L, hd, p);
    if (rc != MOVAE_OK) return rc;
    MOVAE_CHECK_ARG(ws && ws_bytes >= (size_t)B * heads * L * sizeof(float), "movae_attn_bwd: workspace too small");
    float* delta = static_cast<float*>(ws);
    const long rows = (long)B * L;
    const long n = rows * heads;
    long g = (n + 255) / 256;
    g = g > 8192 ? 8192 : g;
    hipLaunchKernelGGL(attn_delta_k, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, out, dout, delta, rows, heads, L, hd, a.oh, a.od);
    MOVAE_CHECK_LAUNCH("attn_delta");
    a.q = q, a.k = k, a.v = v, a.dout = dout, a.lse = lse, a.delta = delta, a.dq = dq, a.dk = dk, a.dv = dv;
    const bool rope = rope_cos != nullptr;
    if (g_movae_compute_bf16) ATTN_LAUNCH_BF(attn_bwd_dkdv_bf_k, a, false, rope, (hipStream_t)stream);
    else ATTN_LAUNCH_BIDIR(attn_bwd_dkdv_k, a, rope, (hipStream_t)stream);
    MOVAE_CHECK_LAUNCH("attn_bwd_dkdv");
    if (g_movae_compute_bf16) ATTN_LAUNCH_BF(attn_bwd_dq_bf_k, a, false, rope, (hipStream_t)stream);
    else ATTN_LAUNCH_BIDIR(attn_bwd_dq_k, a, rope, (hipStream_t)stream);
    MOVAE_CHECK_LAUNCH("attn_bwd_dq");
    return MOVAE_OK;
}

int movae_causal_attn_dropout_mask(uint8_t* keep, int BH, int L, float p, unsigned long long seed, unsigned long long draw,
                                   movae_stream_t stream) {
    MOVAE_CHECK_ARG(keep && BH > 0 && L > 0 && p >= 0.f && p < 1.f, "movae_causal_attn_dropout_mask: bad argument");
    AttnArgs a = AttnArgs{};
    const int rc = setup(a, "movae_causal_attn_dropout_mask", 1, 1, 1, L, 1, p, seed, draw);
    if (rc != MOVAE_OK) return rc;
    const long n4 = (long)BH * L * ((L + 3) / 4);
    long g = (n4 + 255) / 256;
    g = g > 16384 ? 16384 : g;
    hipLaunchKernelGGL(attn_mask_k, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, a, keep, n4);
    MOVAE_CHECK_LAUNCH("causal_attn_dropout_mask");
    return MOVAE_OK;
}

}  // extern "C"
