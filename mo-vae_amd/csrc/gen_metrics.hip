// Feature-space kernels of the generative evaluation (reference main.py:695-887 evaluate_generative_metrics; utils/metrics.py:682-736
// kid_from_features / precision_recall_from_features, :835-914 calculate_inception_score).  Forward only, fp32 operands, no atomics,
// bit-identical from run to run.
//
//   linear_softmax_k     the classifier head: LS_ROWS feature rows per block staged in LDS once, one wave per class reads that class's
//                        weight row with 16-byte loads (scalar loads where D % 4 != 0 or an operand is not 16-byte aligned), every
//                        lane keeps LS_ROWS partial dots, folded with shuffles; the logits stay in LDS and wave r finishes row r:
//                        maximum, sum of expf(l - max), quotient.
//   inception_score_k    one block per split, two phases in one launch: the clipped marginal of the split's rows (one thread per class,
//                        rows in order, fp64) kept in LDS as its logarithm; then sum p (log p - log p_y) over the split in fp64, folded
//                        in a fixed order.
//   kid_subsets_k        one block per subset: the m gathered rows of each set go through LDS in slabs of KID_BK columns; a thread owns
//                        KID_PP (i, j) pairs of the three m x m blocks at a time and keeps their dots in fp64 (fp32 operands widened
//                        before the product, k ascending).  (gamma dot + 1)^degree by repeated multiplication, the diagonals of K_rr
//                        and K_ff skipped, the three sums folded in a fixed order.
//   row_norms_k          |x|^2 per row, one wave per row, fp64 sum rounded once.
//   knn_rows_k<BM, VEC>  squared distances in Gram form on v_mfma_f32_32x32x2_f32, staged like infer_conv_k (inception.hip): BM rows of
//                        a against 64-column tiles of b, 32 k per LDS stage, both operands k-contiguous [row][32 + 4].  One block owns
//                        its rows for ALL column tiles: after a tile's K loop the 2 x 2 waves write |a|^2 + |b|^2 - 2 a.b into an LDS
//                        tile, 256 / BM threads per row each scan a stripe of its columns and keep the 8 smallest in registers (sorted
//                        insertion) with the column of the smallest; the stripes of a row are merged through LDS at the end.
#include "common.h"

#include <math.h>

namespace {

constexpr long long GM_LIMIT = 1LL << 31;
inline bool gm_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- classifier head ---------------------------------------------------------------------------------------------------------------
constexpr int LS_ROWS = 4;  // rows per block = waves per block: wave r finishes row r

template <bool VEC>
__global__ __launch_bounds__(256) void linear_softmax_k(const float* __restrict__ feat, const float* __restrict__ W,
                                                        const float* __restrict__ bias, float* __restrict__ probs, int n, int C, int D) {
    extern __shared__ __attribute__((aligned(16))) float ls_sh[];
    float* fs = ls_sh;                 // [LS_ROWS][D]
    float* lg = ls_sh + LS_ROWS * D;   // [LS_ROWS][C]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r0 = blockIdx.x * LS_ROWS;
    for (int e = t; e < LS_ROWS * D; e += 256) {
        const int r = e / D, row = r0 + r;
        fs[e] = row < n ? feat[(long long)row * D + (e - r * D)] : 0.f;
    }
    __syncthreads();
    for (int c = wave; c < C; c += 4) {
        const float* __restrict__ w = W + (long long)c * D;
        float acc[LS_ROWS];
#pragma unroll
        for (int r = 0; r < LS_ROWS; ++r) acc[r] = 0.f;
        if constexpr (VEC) {
            for (int k = lane * 4; k < D; k += 256) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(w + k);
#pragma unroll
                for (int r = 0; r < LS_ROWS; ++r) {
                    const f32x4 fv = *reinterpret_cast<const f32x4*>(fs + r * D + k);
                    acc[r] = fmaf(wv[0], fv[0], acc[r]);
                    acc[r] = fmaf(wv[1], fv[1], acc[r]);
                    acc[r] = fmaf(wv[2], fv[2], acc[r]);
                    acc[r] = fmaf(wv[3], fv[3], acc[r]);
                }
            }
        } else {
            for (int k = lane; k < D; k += 64) {
                const float wv = w[k];
#pragma unroll
                for (int r = 0; r < LS_ROWS; ++r) acc[r] = fmaf(wv, fs[r * D + k], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < LS_ROWS; ++r) acc[r] = wave_sum(acc[r]);
        if (lane == 0) {
            const float b = bias[c];
#pragma unroll
            for (int r = 0; r < LS_ROWS; ++r) lg[r * C + c] = acc[r] + b;
        }
    }
    __syncthreads();
    const int row = r0 + wave;
    if (row >= n) return;
    const float* l = lg + wave * C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, l[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(l[c] - mx);
    s = wave_sum(s);
    for (int c = lane; c < C; c += 64) probs[(long long)row * C + c] = expf(l[c] - mx) / s;
}

// ---- Inception Score ---------------------------------------------------------------------------------------------------------------
constexpr double IS_EPS = 1e-16;

__device__ __forceinline__ double is_clip(double v) { return v < IS_EPS ? IS_EPS : (v > 1.0 ? 1.0 : v); }

__global__ __launch_bounds__(256) void inception_score_k(const float* __restrict__ probs, int per, int C, double* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) double is_sh[];  // [C] log of the clipped marginal, then 4 doubles of the fold
    double* logpy = is_sh;
    double* fold = is_sh + C;
    const int t = threadIdx.x;
    const float* __restrict__ part = probs + (long long)blockIdx.x * per * C;
    for (int c = t; c < C; c += 256) {
        double s = 0.0;
        for (int r = 0; r < per; ++r) s += is_clip((double)part[(long long)r * C + c]);
        logpy[c] = log(is_clip(s / (double)per));
    }
    __syncthreads();
    double kl = 0.0;
    const long long total = (long long)per * C;
    for (long long e = t; e < total; e += 256) {
        const double p = is_clip((double)part[e]);
        kl += p * (log(p) - logpy[(int)(e % C)]);
    }
    kl = block_sum_256(kl, fold);
    if (t == 0) scores[blockIdx.x] = exp(kl / (double)per);
}

// ---- KID ---------------------------------------------------------------------------------------------------------------------------
constexpr int KID_BK = 32;            // columns per LDS slab
constexpr int KID_LD = KID_BK + 1;    // floats per LDS row (odd: consecutive rows fall on consecutive banks)
constexpr int KID_PP = 8;             // (i, j) pairs a thread owns at a time
constexpr int KID_MAX_M = 240;        // 2 * m * KID_LD floats must fit 64 KB

__device__ __forceinline__ double kid_poly(double dot, double gamma, int degree) {
    const double b = gamma * dot + 1.0;
    double v = 1.0;
    for (int q = 0; q < degree; ++q) v *= b;
    return v;
}

__global__ __launch_bounds__(256) void kid_subsets_k(const float* __restrict__ real, const float* __restrict__ fake,
                                                     const int* __restrict__ idx_real, const int* __restrict__ idx_fake, int nr, int nf,
                                                     int m, int D, double gamma, int degree, double* __restrict__ mmd2) {
    extern __shared__ __attribute__((aligned(16))) float kid_sh[];
    float* Rs = kid_sh;               // [m][KID_LD]
    float* Fs = kid_sh + m * KID_LD;  // [m][KID_LD]
    __shared__ double fold[4];
    const int t = threadIdx.x;
    const int* __restrict__ ir = idx_real + (long long)blockIdx.x * m;
    const int* __restrict__ jf = idx_fake + (long long)blockIdx.x * m;
    const int pairs = m * m;
    double srr = 0.0, sff = 0.0, srf = 0.0;
    for (int p0 = 0; p0 < pairs; p0 += 256 * KID_PP) {
        double rr[KID_PP], ff[KID_PP], rf[KID_PP];
        int pi[KID_PP], pj[KID_PP];
#pragma unroll
        for (int q = 0; q < KID_PP; ++q) {
            rr[q] = ff[q] = rf[q] = 0.0;
            const int p = p0 + q * 256 + t;
            const int pp = p < pairs ? p : 0;  // (a pair past the end computes pair 0 and is not summed)
            pi[q] = (pp / m) * KID_LD;
            pj[q] = (pp % m) * KID_LD;
        }
        for (int k0 = 0; k0 < D; k0 += KID_BK) {
            __syncthreads();  // the previous slab has been consumed
            for (int e = t; e < m * KID_BK; e += 256) {
                const int row = e / KID_BK, kk = e - row * KID_BK, k = k0 + kk;
                const int a = ir[row], b = jf[row];
                // (an index outside its set reads nothing: the caller validates them; this keeps a bad one from faulting)
                Rs[row * KID_LD + kk] = (k < D && (unsigned)a < (unsigned)nr) ? real[(long long)a * D + k] : 0.f;
                Fs[row * KID_LD + kk] = (k < D && (unsigned)b < (unsigned)nf) ? fake[(long long)b * D + k] : 0.f;
            }
            __syncthreads();
            for (int kk = 0; kk < KID_BK; ++kk) {
#pragma unroll
                for (int q = 0; q < KID_PP; ++q) {
                    const double ri = (double)Rs[pi[q] + kk], rj = (double)Rs[pj[q] + kk];
                    const double fi = (double)Fs[pi[q] + kk], fj = (double)Fs[pj[q] + kk];
                    rr[q] = fma(ri, rj, rr[q]);
                    ff[q] = fma(fi, fj, ff[q]);
                    rf[q] = fma(ri, fj, rf[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < KID_PP; ++q) {
            const int p = p0 + q * 256 + t;
            if (p < pairs) {
                srf += kid_poly(rf[q], gamma, degree);
                if (pi[q] != pj[q]) {
                    srr += kid_poly(rr[q], gamma, degree);
                    sff += kid_poly(ff[q], gamma, degree);
                }
            }
        }
    }
    srr = block_sum_256(srr, fold);
    sff = block_sum_256(sff, fold);
    srf = block_sum_256(srf, fold);
    if (t == 0) {
        const double off = (double)m * (double)(m - 1);
        const double v = srr / off + sff / off - 2.0 * (srf / ((double)m * (double)m));
        mmd2[blockIdx.x] = v > 0.0 ? v : 0.0;
    }
}

// ---- nearest neighbours ------------------------------------------------------------------------------------------------------------
constexpr int KN_BK = 32;
constexpr int KN_LDR = KN_BK + 4;   // floats per LDS operand row
constexpr int KN_BN = 64;           // columns of b per tile
constexpr int KN_LDD = KN_BN + 1;   // floats per row of the distance tile
constexpr int KN_K = 8;             // the list every scanning thread keeps

__global__ __launch_bounds__(256) void row_norms_k(const float* __restrict__ x, float* __restrict__ out, int n, int D) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* __restrict__ xr = x + (long long)row * D;
    double s = 0.0;
    for (int k = lane; k < D; k += 64) s += (double)xr[k] * (double)xr[k];
    s = wave_sum(s);
    if (lane == 0) out[row] = (float)s;
}

// sorted insertion of d into best[0] <= ... <= best[7]; `col` replaces idx0 when d becomes the smallest (a tie goes to the smaller
// column)
__device__ __forceinline__ void kn_insert(float (&best)[KN_K], int& idx0, float d, int col) {
    if (d < best[0] || (d == best[0] && col < idx0)) idx0 = col;
    if (!(d < best[KN_K - 1])) return;
#pragma unroll
    for (int q = KN_K - 1; q > 0; --q) best[q] = d < best[q - 1] ? best[q - 1] : (d < best[q] ? d : best[q]);
    best[0] = d < best[0] ? d : best[0];
}

struct KnnP {
    const float* a;
    const float* b;
    const float* a2;
    const float* b2;
    float* dist2;
    int* idx;
    int na, nb, D, k, exclude_diag;
};

template <int BM, bool VEC>
__global__ __launch_bounds__(256) void knn_rows_k(KnnP p) {
    constexpr int TM = BM / 64;       // 2 x 2 waves, each 32 TM rows x 32 columns
    constexpr int AC = BM / 32, BC = KN_BN / 32;
    constexpr int TPR = 256 / BM;     // scanning threads per row
    constexpr int STRIPE = KN_BN / TPR;
    __shared__ __attribute__((aligned(16))) float As[BM * KN_LDR];
    __shared__ __attribute__((aligned(16))) float Bs[KN_BN * KN_LDR];
    __shared__ float Dt[BM * KN_LDD];
    __shared__ float An[BM], Bn[KN_BN];
    static_assert(256 * (KN_K + 1) <= BM * KN_LDD, "the merge lists reuse the distance tile");
    const float* __restrict__ A = p.a;
    const float* __restrict__ B = p.b;
    const int t = threadIdx.x, lane = t & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = t >> 6, wm = wave >> 1, wn = wave & 1;
    const int kq = t & 7, r8 = t >> 3;
    const int m0 = blockIdx.x * BM;
    const int D = p.D, na = p.na, nb = p.nb;

    long long a_base[AC];
    bool a_ok[AC];
#pragma unroll
    for (int i = 0; i < AC; ++i) {
        const int m = m0 + r8 + 32 * i;
        a_ok[i] = m < na;
        a_base[i] = (long long)(a_ok[i] ? m : 0) * D;
    }
    if (t < BM) An[t] = m0 + t < na ? p.a2[m0 + t] : 0.f;

    // the scanning role of this thread: row srow of the tile, columns sstripe .. sstripe + STRIPE - 1 of every column tile
    const int srow = t % BM, sstripe = (t / BM) * STRIPE;
    const int grow = m0 + srow;
    float best[KN_K];
    int idx0 = 0;
#pragma unroll
    for (int q = 0; q < KN_K; ++q) best[q] = INFINITY;

    const int nk = (D + KN_BK - 1) / KN_BK;
    for (int n0 = 0; n0 < nb; n0 += KN_BN) {
        long long b_base[BC];
        bool b_ok[BC];
#pragma unroll
        for (int i = 0; i < BC; ++i) {
            const int n = n0 + r8 + 32 * i;
            b_ok[i] = n < nb;
            b_base[i] = (long long)(b_ok[i] ? n : 0) * D;
        }
        if (t < KN_BN) Bn[t] = n0 + t < nb ? p.b2[n0 + t] : 0.f;  // (read after the K loop's barriers)

        f32x4 ra[AC], rb[BC];
        auto load_tile = [&](int kt) {
            const int k = kt * KN_BK + kq * 4;
#pragma unroll
            for (int i = 0; i < AC; ++i) ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < BC; ++i) rb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (VEC) {  // D % 4 == 0: the chunk is whole or past the end
                if (k < D) {
#pragma unroll
                    for (int i = 0; i < AC; ++i)
                        if (a_ok[i]) ra[i] = *reinterpret_cast<const f32x4*>(A + (a_base[i] + k));
#pragma unroll
                    for (int i = 0; i < BC; ++i)
                        if (b_ok[i]) rb[i] = *reinterpret_cast<const f32x4*>(B + (b_base[i] + k));
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int ke = k + e;
                    if (ke >= D) continue;
#pragma unroll
                    for (int i = 0; i < AC; ++i)
                        if (a_ok[i]) ra[i][e] = A[a_base[i] + ke];
#pragma unroll
                    for (int i = 0; i < BC; ++i)
                        if (b_ok[i]) rb[i][e] = B[b_base[i] + ke];
                }
            }
        };
        auto store_tile = [&]() {
#pragma unroll
            for (int i = 0; i < AC; ++i) *reinterpret_cast<f32x4*>(As + (r8 + 32 * i) * KN_LDR + kq * 4) = ra[i];
#pragma unroll
            for (int i = 0; i < BC; ++i) *reinterpret_cast<f32x4*>(Bs + (r8 + 32 * i) * KN_LDR + kq * 4) = rb[i];
        };

        f32x16 acc[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

        load_tile(0);
        store_tile();
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const bool more = kt + 1 < nk;  // (block-uniform)
            if (more) load_tile(kt + 1);
#pragma unroll
            for (int jj = 0; jj < KN_BK / 8; ++jj) {
                f32x4 a4[TM];
                const f32x4 b4 = *reinterpret_cast<const f32x4*>(Bs + (wn * 32 + l31) * KN_LDR + half * (KN_BK / 2) + jj * 4);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
                    a4[tm] = *reinterpret_cast<const f32x4*>(As + (wm * TM * 32 + tm * 32 + l31) * KN_LDR + half * (KN_BK / 2) + jj * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) acc[tm] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[tm][e], b4[e], acc[tm], 0, 0, 0);
            }
            __syncthreads();
            if (more) {
                store_tile();
                __syncthreads();
            }
        }

        // accumulator register r of a lane: row (r & 3) + 8 (r >> 2) + 4 half of its 32 x 32 tile, column lane & 31
        {
            const int cl = wn * 32 + l31;
            const float b2 = Bn[cl];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = wm * TM * 32 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    Dt[rl * KN_LDD + cl] = (An[rl] + b2) - 2.f * acc[tm][r];
                }
        }
        __syncthreads();
        if (grow < na) {
#pragma unroll 4
            for (int j = 0; j < STRIPE; ++j) {
                const int col = n0 + sstripe + j;
                if (col < nb && !(p.exclude_diag && col == grow)) kn_insert(best, idx0, Dt[srow * KN_LDD + sstripe + j], col);
            }
        }
        // (the next tile writes Dt only behind the barriers of its K loop, and As / Bs only after every wave has passed the one above)
    }

    // merge the TPR stripes of a row: stripe 0's thread takes the others' lists in column order
    __syncthreads();
    float* lists = Dt;  // [256][KN_K + 1]
#pragma unroll
    for (int q = 0; q < KN_K; ++q) lists[t * (KN_K + 1) + q] = best[q];
    lists[t * (KN_K + 1) + KN_K] = __int_as_float(idx0);
    __syncthreads();
    if (t < BM && grow < na) {
        for (int s = 1; s < TPR; ++s) {
            const float* o = lists + (s * BM + srow) * (KN_K + 1);
            const int oi = __float_as_int(o[KN_K]);
#pragma unroll
            for (int q = 0; q < KN_K; ++q) kn_insert(best, idx0, o[q], oi);
        }
#pragma unroll
        for (int q = 0; q < KN_K; ++q)
            if (q < p.k) p.dist2[(long long)grow * p.k + q] = fmaxf(best[q], 0.f);
        p.idx[grow] = idx0;
    }
}

template <int BM>
void launch_knn(const KnnP& p, bool vec, hipStream_t st) {
    const dim3 grid((p.na + BM - 1) / BM), block(256);
    if (vec) hipLaunchKernelGGL((knn_rows_k<BM, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((knn_rows_k<BM, false>), grid, block, 0, st, p);
}

}  // namespace

extern "C" int movae_linear_softmax(const float* feat, const float* weight, const float* bias, float* probs, int n, int C, int D,
                                    movae_stream_t stream) {
    MOVAE_CHECK_ARG(feat && weight && bias && probs, "movae_linear_softmax: null pointer");
    MOVAE_CHECK_ARG(n > 0 && C > 0 && D > 0, "movae_linear_softmax: empty shape n %d C %d D %d", n, C, D);
    MOVAE_CHECK_ARG((long long)n * D < GM_LIMIT && (long long)n * C < GM_LIMIT && (long long)C * D < GM_LIMIT,
                    "movae_linear_softmax: the shape is too large (n %d C %d D %d)", n, C, D);
    const size_t lds = (size_t)LS_ROWS * ((size_t)D + (size_t)C) * sizeof(float);
    MOVAE_CHECK_ARG(lds <= 64 * 1024, "movae_linear_softmax: %d rows of D %d + C %d floats do not fit 64 KB of LDS", LS_ROWS, D, C);
    const dim3 grid((n + LS_ROWS - 1) / LS_ROWS), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (D % 4 == 0 && gm_aligned16(weight)) hipLaunchKernelGGL((linear_softmax_k<true>), grid, block, lds, st, feat, weight, bias, probs, n, C, D);
    else hipLaunchKernelGGL((linear_softmax_k<false>), grid, block, lds, st, feat, weight, bias, probs, n, C, D);
    MOVAE_CHECK_LAUNCH("linear_softmax_k");
    return MOVAE_OK;
}

extern "C" int movae_inception_score(const float* probs, int n, int C, int splits, double* scores, movae_stream_t stream) {
    MOVAE_CHECK_ARG(probs && scores, "movae_inception_score: null pointer");
    MOVAE_CHECK_ARG(n > 0 && C > 0 && splits > 0, "movae_inception_score: empty shape n %d C %d splits %d", n, C, splits);
    MOVAE_CHECK_ARG(n / splits >= 1, "movae_inception_score: %d rows leave every one of %d splits empty", n, splits);
    MOVAE_CHECK_ARG((long long)n * C < GM_LIMIT * 4 && C <= 7000, "movae_inception_score: the shape is too large (n %d C %d)", n, C);
    MOVAE_CHECK_ARG((reinterpret_cast<uintptr_t>(scores) & 7) == 0, "movae_inception_score: scores must be 8-byte aligned");
    const size_t lds = ((size_t)C + 4) * sizeof(double);
    hipLaunchKernelGGL(inception_score_k, dim3(splits), dim3(256), lds, static_cast<hipStream_t>(stream), probs, n / splits, C, scores);
    MOVAE_CHECK_LAUNCH("inception_score_k");
    return MOVAE_OK;
}

extern "C" int movae_kid_subsets(const float* real, const float* fake, const int* idx_real, const int* idx_fake, int nr, int nf, int S, int m,
                                 int D, double gamma, int degree, double* mmd2, movae_stream_t stream) {
    MOVAE_CHECK_ARG(real && fake && idx_real && idx_fake && mmd2, "movae_kid_subsets: null pointer");
    MOVAE_CHECK_ARG(nr > 0 && nf > 0 && S > 0 && D > 0, "movae_kid_subsets: empty shape nr %d nf %d S %d D %d", nr, nf, S, D);
    MOVAE_CHECK_ARG(m >= 2 && m <= KID_MAX_M, "movae_kid_subsets: subset size %d (2 .. %d)", m, KID_MAX_M);
    MOVAE_CHECK_ARG(m <= nr && m <= nf, "movae_kid_subsets: subset size %d above a set's size (%d, %d)", m, nr, nf);
    MOVAE_CHECK_ARG(degree >= 1 && degree <= 16, "movae_kid_subsets: degree %d (1 .. 16)", degree);
    MOVAE_CHECK_ARG((long long)nr * D < GM_LIMIT * 4 && (long long)nf * D < GM_LIMIT * 4 && (long long)S * m < GM_LIMIT,
                    "movae_kid_subsets: the shape is too large");
    MOVAE_CHECK_ARG((reinterpret_cast<uintptr_t>(mmd2) & 7) == 0, "movae_kid_subsets: mmd2 must be 8-byte aligned");
    const size_t lds = (size_t)2 * m * KID_LD * sizeof(float);
    hipLaunchKernelGGL(kid_subsets_k, dim3(S), dim3(256), lds, static_cast<hipStream_t>(stream), real, fake, idx_real, idx_fake, nr, nf, m, D,
                       gamma, degree, mmd2);
    MOVAE_CHECK_LAUNCH("kid_subsets_k");
    return MOVAE_OK;
}

extern "C" int movae_knn_rows(const float* a, const float* b, int na, int nb, int D, int k, int exclude_diag, int tile, float* norms,
                              float* dist2, int* idx, movae_stream_t stream) {
    MOVAE_CHECK_ARG(a && b && norms && dist2 && idx, "movae_knn_rows: null pointer");
    MOVAE_CHECK_ARG(na > 0 && nb > 0 && D > 0, "movae_knn_rows: empty shape na %d nb %d D %d", na, nb, D);
    MOVAE_CHECK_ARG(k >= 1 && k <= KN_K, "movae_knn_rows: k %d (1 .. %d)", k, KN_K);
    MOVAE_CHECK_ARG(exclude_diag == 0 || exclude_diag == 1, "movae_knn_rows: exclude_diag %d", exclude_diag);
    MOVAE_CHECK_ARG(nb - exclude_diag >= k, "movae_knn_rows: %d candidates per row are fewer than k %d", nb - exclude_diag, k);
    MOVAE_CHECK_ARG(tile == 0 || tile == 64 || tile == 128, "movae_knn_rows: tile %d (0 = chosen here, 64, 128)", tile);
    MOVAE_CHECK_ARG((long long)na * D < GM_LIMIT * 4 && (long long)nb * D < GM_LIMIT * 4 && (long long)na * k < GM_LIMIT,
                    "movae_knn_rows: the shape is too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(row_norms_k, dim3((na + 3) / 4), dim3(256), 0, st, a, norms, na, D);
    hipLaunchKernelGGL(row_norms_k, dim3((nb + 3) / 4), dim3(256), 0, st, b, norms + na, nb, D);
    MOVAE_CHECK_LAUNCH("row_norms_k");
    KnnP p{a, b, norms, norms + na, dist2, idx, na, nb, D, k, exclude_diag};
    const bool vec = D % 4 == 0 && gm_aligned16(a) && gm_aligned16(b);
    // 128 rows per block once that still gives every compute unit a block; below that the 64-row tile spreads the rows further
    const int bm = tile ? tile : ((na + 127) / 128 >= 256 ? 128 : 64);
    if (bm == 128) launch_knn<128>(p, vec, st);
    else launch_knn<64>(p, vec, st);
    MOVAE_CHECK_LAUNCH("knn_rows_k");
    return MOVAE_OK;
}
