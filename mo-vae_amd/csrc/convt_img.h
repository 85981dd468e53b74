// convt_img.h -- whole-image-row forward kernel for the decoder's 3x3 stride-2 transposed conv with 32 input and 32 output
// channels (included inside conv_igemm.hip's anonymous namespace, after kgemm.h).  DESIGN.md section 3.1.
//
// The tiled BWD form cuts such a layer into four output-parity classes of 128 x 32 blocks whose reductions are 1 / 2 / 2 / 4 taps
// of 32 channels: 1-4 k-stages, all prologue and epilogue, every input pixel fetched once per class, 128-byte stores at a
// 256-byte stride.  Here the input is stationary.  A GROUP is 32 consecutive input pixels = whole rows of one image (wi 8: four
// rows, wi 16: two); a block owns four groups, a wave one.  Output pixel (2i + dh, 2j + dw) of class (dh, dw) reads
//   (0,0): x[i][j] w[1][1]
//   (0,1): x[i][j+1] w[1][0] + x[i][j] w[1][2]
//   (1,0): x[i+1][j] w[0][1] + x[i][j] w[2][1]
//   (1,1): x[i+1][j+1] w[0][0] + x[i+1][j] w[0][2] + x[i][j+1] w[2][0] + x[i][j] w[2][2]
// so a wave multiplies its group's 32 pixels, read from LDS at the four shifts (0,0) (0,1) (1,0) (1,1), into one 32x32
// accumulator per class (v_mfma_f32_32x32x2_f32).  A block stages, once: all weights [32][3][3][32] as they lie in memory, and
// per group its rows plus the row below and the column to the right (exact zero outside the image; the producer's BatchNorm +
// LeakyReLU applied to in-image elements while staging).
//
// SAME BITS AS THE TILED KERNEL.  A training step amplifies a last-bit difference in these layers to the third digit of the loss
// within twenty steps, so the kernel reproduces igemm2_bwd<128,32> (unsplit, as it runs at these shapes) bit for bit:
//   * an output element is ONE chain of MFMAs: the class's taps in the order above (igemm2_bwd_body's (ta, tb) order), per tap
//     sixteen steps j = 0..15 whose lane halves carry channels j and 16 + j (mma_rk's k order inside a 32-deep stage);
//   * bias is added to the finished sum, then the activation;
//   * statistics: the tiled kernel emits one partial pair per (class, 128-row block), a block's rows being 128 consecutive
//     pixels = this kernel's four groups; for a column, q[i] = ((v[i] + v[32 + i]) + v[64 + i]) + v[96 + i] (rows past the end
//     skipped), then q[0] + q[1] + ... + q[31] from zero, squares through fmaf likewise (tile_epilogue's side_lds path).  The
//     four classes meet in LDS after the stores and are folded in exactly that order into slot class * blocks + block.
// The wave runs classes (0,0) + (0,1) (three taps), stores them straight from the registers -- a half-wave holds the 32 channels
// of one output pixel, a whole 128-byte line -- then (1,0) + (1,1) (six taps): the first stores drain under the second pass.
#pragma once

namespace img {

constexpr int CI = 32;       // input channels
constexpr int GPB = 4;       // groups per block
constexpr int LDX = 57;      // floats between the channels of a group's staged pixels: >= 3 * 17 positions; 57 % 8 == 1 spreads
                             // the four-channel staging stores of neighbouring lanes over the banks
constexpr int OUT_G = 4096;  // floats of a group's output: 32 pixels * 4 classes * 32 channels
constexpr int WROW = 288;    // floats of one input channel's weights: 3 * 3 * 32
constexpr int XIT = 7;       // staging trips: groups per block * positions * (ci / 4) <= 1632 = 4 * 51 * 8
constexpr int MAIN = CI * WROW + GPB * CI * LDX;  // floats: weights, then the groups' pixels; afterwards the statistics tile
constexpr int LDS_BYTES = MAIN * 4;
static_assert(MAIN >= 4 * 128 * 32, "the four classes' 128 x 32 tiles fit the operand memory");

struct ImgArgs {
    const float* X;
    const float* W;
    float* Y;
    const float* bias;
    int act;
    float slope;
    Norm nrm;
    float* stats;  // [4 classes][blocks][2][32] or null
    int groups;    // 32-pixel groups in all
    int hi;
    FastDiv fd_gpi;  // by the groups per image
};

// taps of class c in the tiled kernel's order: weight tap kh * 3 + kw and the shift of the pixel it multiplies (bit 0: column + 1,
// bit 1: row + 1)
__device__ constexpr int NTAP[4] = {1, 2, 2, 4};
__device__ constexpr int TAP[4][4] = {{4, 0, 0, 0}, {3, 5, 0, 0}, {1, 7, 0, 0}, {0, 2, 6, 8}};
__device__ constexpr int SHIFT[4][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, 0, 0, 0}, {3, 2, 1, 0}};

// classes CA and CB of the wave's group: xa = the lane's pixel in channel 16 * half, wb = the lane's column in that channel
template <int CA, int CB, int PW>
__device__ __forceinline__ void img_mma(const float* __restrict__ xa, const float* __restrict__ wb, f32x16 (&acc)[4]) {
    constexpr int SA = NTAP[CA] * 16, STEPS = SA + NTAP[CB] * 16;
    constexpr int D = 4;  // steps of operands in flight: an LDS read takes longer than one 16-pass MFMA
    float a[D], b[D];
    auto fetch = [&](int st, int s) {  // step st: (class, tap, j)
        const int c = st < SA ? CA : CB, u = st < SA ? st : st - SA;
        const int i = u >> 4, j = u & 15;
        const int sh = SHIFT[c][i];
        a[s] = xa[j * LDX + (sh & 1) + (sh >> 1) * PW];
        b[s] = wb[j * WROW + TAP[c][i] * 32];
    };
#pragma unroll
    for (int st = 0; st < D - 1; ++st) fetch(st, st);
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
        const int s = st % D;
        if (st + D - 1 < STEPS) fetch(st + D - 1, (st + D - 1) % D);  // later steps' operands leave LDS ahead of this step's MFMA ...
        __builtin_amdgcn_sched_barrier(0);  // ... (left alone, the scheduler sinks each read to just above its MFMA)
        if (st < SA) acc[CA] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc[CA], 0, 0, 0);
        else acc[CB] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc[CB], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// classes CA and CB, with bias and activation, into the group's output rows yg[2 * rows][2 * wi][32] (yg: the lane's column);
// acc keeps what was stored
template <int CA, int CB, int LW, bool ACT>
__device__ __forceinline__ void img_store(float* __restrict__ yg, f32x16 (&acc)[4], float bias, int act, float slope, int half) {
    constexpr int wi = 1 << LW;
    yg += half * 2 * 4 * 32;  // (row 4 * half of the MFMA tile is four pixels to the right: the rest are constants)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = k ? CB : CA;
        const int dh = c >> 1, dw = c & 1;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = acc_row(r, 0);
            const int pr = p >> LW, pc = p & (wi - 1);
            float v = acc[c][r] + bias;
            if (ACT) v = v > 0.f ? v : (act == MOVAE_ACT_RELU ? 0.f : v * slope);  // (the gate admits LeakyReLU and ReLU only)
            acc[c][r] = v;
            yg[((2 * pr + dh) * 2 * wi + 2 * pc + dw) * 32] = v;
        }
    }
}

template <int LW>
__global__ __launch_bounds__(256) void igemm2_bwd_img(ImgArgs a) {
    constexpr int Q = CI / 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const wsm = lds;               // [CI][3][3][32]
    float* const xsm = lds + CI * WROW;   // [GPB][CI][LDX]
    const int t = threadIdx.x;
    const int g0 = blockIdx.x * GPB;
    constexpr int wi = 1 << LW, R = 32 >> LW, pw = wi + 1;  // image width, rows of a group, staged row pitch
    constexpr int gitems = (R + 1) * pw * Q;
    const int hi = a.hi;
    const int q = t & (Q - 1);  // (Q divides 256: a thread keeps its channel quad over the trips)

    // ---- stage: the weights and the pixels of the block's groups, every load issued before the first LDS store -------------
    constexpr int WIT = CI * WROW / 4 / 256;  // sixteen-byte pieces per thread
    f32x4 wv[WIT];
#pragma unroll
    for (int i = 0; i < WIT; ++i) wv[i] = reinterpret_cast<const f32x4*>(a.W)[i * 256 + t];
    f32x4 xv[XIT];
    int xoff[XIT];  // float offset into xsm, -1: nothing to store
    bool xin[XIT];  // the position lies inside the image
#pragma unroll
    for (int i = 0; i < XIT; ++i) {
        const int idx = t + i * 256;
        const int g = idx / gitems;
        const int pos = (idx - g * gitems) / Q;
        const int r = pos / pw, c = pos - r * pw;
        const int gi = g0 + g;
        const int im = fdiv(gi, a.fd_gpi);
        const int row = (gi - im * (hi >> (5 - LW))) * R + r;  // (hi * wi / 32 groups per image)
        const bool in_block = g < GPB;
        const bool valid = in_block && gi < a.groups && row < hi && c < wi;
        xoff[i] = in_block ? (g * CI + 4 * q) * LDX + pos : -1;
        xin[i] = valid;
        xv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (valid) xv[i] = *reinterpret_cast<const f32x4*>(a.X + (((size_t)im * hi + row) * wi + c) * CI + 4 * q);
    }
    if (a.nrm.scale) {  // the producer's BatchNorm + LeakyReLU, on in-image elements only: the padding stays exact zero
        const f32x4 sc = *reinterpret_cast<const f32x4*>(a.nrm.scale + 4 * q), sh = *reinterpret_cast<const f32x4*>(a.nrm.shift + 4 * q);
#pragma unroll
        for (int i = 0; i < XIT; ++i) xv[i] = norm_apply_if(xin[i], xv[i], sc, sh, a.nrm.slope);
    }
#pragma unroll
    for (int i = 0; i < XIT; ++i) {
        if (xoff[i] >= 0) {
            float* d = xsm + xoff[i];
            d[0] = xv[i][0], d[LDX] = xv[i][1], d[2 * LDX] = xv[i][2], d[3 * LDX] = xv[i][3];
        }
    }
#pragma unroll
    for (int i = 0; i < WIT; ++i) reinterpret_cast<f32x4*>(wsm)[i * 256 + t] = wv[i];
    __syncthreads();

    // ---- multiply and store ---------------------------------------------------------------------------------------------------
    const int g = t >> 6, lane = t & 63, half = lane >> 5, l31 = lane & 31;  // the wave's group
    const bool live = g0 + g < a.groups;  // (wave-uniform; the last block may have fewer groups)
    f32x16 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    if (live) {
        const float* xa = xsm + (g * CI + half * 16) * LDX + (l31 >> LW) * pw + (l31 & (wi - 1));
        const float* wb = wsm + half * 16 * WROW + l31;
        float* const yg = a.Y + (size_t)(g0 + g) * OUT_G + l31;
        const float bias = a.bias ? a.bias[l31] : 0.f;
        const bool plain = a.act == MOVAE_ACT_NONE;  // (uniform)
        img_mma<0, 1, pw>(xa, wb, acc);
        if (plain) img_store<0, 1, LW, false>(yg, acc, bias, a.act, a.slope, half);
        else img_store<0, 1, LW, true>(yg, acc, bias, a.act, a.slope, half);
        img_mma<2, 3, pw>(xa, wb, acc);
        if (plain) img_store<2, 3, LW, false>(yg, acc, bias, a.act, a.slope, half);
        else img_store<2, 3, LW, true>(yg, acc, bias, a.act, a.slope, half);
    }
    if (!a.stats) return;  // (uniform)

    // ---- statistics: the tiled kernel's partials, value for value (see the head of this file) -----------------------------------
    __syncthreads();  // every wave is done with the operands: the classes' 128 x 32 tiles of stored values take their place
    float* const S = lds;  // [class][128 rows][32]
    if (live) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) S[(c * 128 + g * 32 + acc_row(r, half)) * 32 + l31] = acc[c][r];
    }
    __syncthreads();
    const int nlive = a.groups - g0 < GPB ? a.groups - g0 : GPB;
    const int cq = t & 7, rowi = t >> 3;
    f32x4 s1[4], s2[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        s1[c] = f32x4{0.f, 0.f, 0.f, 0.f}, s2[c] = s1[c];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (u < nlive) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(S + (c * 128 + rowi + 32 * u) * 32 + cq * 4);
                s1[c] += v;
#pragma unroll
                for (int j = 0; j < 4; ++j) s2[c][j] = fmaf(v[j], v[j], s2[c][j]);
            }
        }
    }
    __syncthreads();
    float* const F = lds;  // [class][sum | sum of squares][32 row lanes][32]
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        *reinterpret_cast<f32x4*>(F + ((c * 2 + 0) * 32 + rowi) * 32 + cq * 4) = s1[c];
        *reinterpret_cast<f32x4*>(F + ((c * 2 + 1) * 32 + rowi) * 32 + cq * 4) = s2[c];
    }
    __syncthreads();
    if (t < 128) {
        const int c = t >> 5, col = t & 31;
        float c1 = 0.f, c2 = 0.f;
        for (int i = 0; i < 32; ++i) c1 += F[((c * 2 + 0) * 32 + i) * 32 + col], c2 += F[((c * 2 + 1) * 32 + i) * 32 + col];
        const size_t pidx = (size_t)c * gridDim.x + blockIdx.x;
        a.stats[(pidx * 2 + 0) * 32 + col] = c1;
        a.stats[(pidx * 2 + 1) * 32 + col] = c2;
    }
}

template <int LW>
inline int launch_img_t(const ImgArgs& a, hipStream_t st) {
    static bool lds_set = false;
    if (!lds_set) {  // above 64 KB of dynamic LDS a kernel has to ask once
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(igemm2_bwd_img<LW>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) !=
            hipSuccess) {
            (void)hipGetLastError();
            movae_set_error("igemm2_bwd_img: %d bytes of LDS refused", LDS_BYTES);
            return MOVAE_EUNSUPPORTED;
        }
        lds_set = true;
    }
    hipLaunchKernelGGL((igemm2_bwd_img<LW>), dim3((unsigned)ceil_div(a.groups, GPB)), dim3(256), LDS_BYTES, st, a);
    MOVAE_CHECK_LAUNCH("igemm2_bwd_img");
    return MOVAE_OK;
}

// the gate; g is the BWD-form geometry of a transposed conv's FORWARD pass
inline bool img_ok(const float* X, const float* W, const float* Y, const Geom& g, const Epilogue& ep) {
    const long px = (long)g.Hi * g.Wi;
    return g.KH == 3 && g.KW == 3 && g.stride == 2 && g.pad == 1 && g.Ho == 2 * g.Hi && g.Wo == 2 * g.Wi && g.Nn == 32 && g.Cr == CI &&
           (g.Wi == 8 || g.Wi == 16) && px % 32 == 0 && px <= 256 && kg::al16(X) && kg::al16(W) && kg::al16(Y) && kg::al16(ep.bias) &&
           kg::al16(g_fuse.nrm.scale) && kg::al16(g_fuse.nrm.shift) && !g_movae_compute_bf16 && !g_fuse.am.y && !g_fuse.am.res && !g_fuse.bn_y &&
           (ep.act == MOVAE_ACT_NONE || ep.act == MOVAE_ACT_LRELU || ep.act == MOVAE_ACT_RELU) && (long)g.Nimg * px / 32 <= 0x3fffffffL;
}

inline int launch_img(const float* X, const float* W, float* Y, const Geom& g, const Epilogue& ep, hipStream_t st) {
    if (int rc = defer_flush()) return rc;  // not a carrier: a parked weight-gradient reduce goes first, on its own
    ImgArgs a{};
    a.X = X, a.W = W, a.Y = Y, a.bias = ep.bias, a.act = ep.act, a.slope = ep.slope, a.nrm = g_fuse.nrm;
    a.groups = (int)((long)g.Nimg * g.Hi * g.Wi / 32);
    a.hi = g.Hi;
    a.fd_gpi = fastdiv_make(g.Hi * g.Wi / 32);
    // the tiled kernel's partial layout: (class, 128-row block), classes * blocks pairs
    if (g_fuse.stats && ep.act == MOVAE_ACT_NONE) a.stats = fuse_stats_claim(4L * ceil_div(a.groups, GPB), 32);
    g_last_kernel = "igemm2_bwd_img<32>";  // (the image width, 8 or 16, is the kernel's template parameter)
    return g.Wi == 8 ? launch_img_t<3>(a, st) : launch_img_t<4>(a, st);
}

}  // namespace img
