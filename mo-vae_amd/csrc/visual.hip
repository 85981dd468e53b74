// Image grids as bytes: a float image batch [n][c][h][w] (any strides) -> the finished uint8 picture [H][W][3] of torchvision's
// make_grid followed by save_image's quantisation (reference main.py:511-656 builds every figure that way; the geometry and the
// arithmetic are restated in include/movae.h).  The images never leave the device as floats: what the host copies is the picture.
//
// One launch for MOVAE_GRID_RAW / MOVAE_GRID_RANGE, two for MOVAE_GRID_MINMAX:
//   grid_minmax_k   per-block (min, max) partials of the whole batch into the workspace
//   grid_u8_k       output-indexed: a thread owns one aligned 4-byte word of one grid row (the bytes of it that lie inside the row),
//                   finds for each byte its cell, image, channel and pixel, or the padding, and stores the word whole where all four
//                   bytes are the row's, byte by byte at the ragged ends (a row is 3 W bytes, usually no multiple of 4).  In mode
//                   MINMAX every block first folds the partials (at most MM_BLOCKS, fewer than one per thread) itself.
// No atomics, no host read, no second pass over the workspace; min and max do not depend on the fold order, so the bytes are the
// same from run to run.
//
// The per-pixel arithmetic must give torch's bytes: every operation is rounded on its own (no contraction of v * 255 + 0.5 into an
// fma) and the normalisation divides (an IEEE division; a multiplication by the reciprocal gives other bytes).
#include "common.h"

#include <math.h>

namespace {

constexpr int GT = 256;         // threads per block, both kernels
constexpr int MM_BLOCKS = 256;  // cap of the min / max pass's grid: the grid kernel folds the partials with one thread each
constexpr int MM_UNROLL = 4;    // elements per thread in flight at once

struct Strides {
    long long n, c, h, w;
};

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

// dense != 0: the strides are a permutation of a packed layout, so the elements are the `total` floats from x on
__global__ __launch_bounds__(GT) void grid_minmax_k(const float* __restrict__ x, Strides s, int dense, int C, int H, int W,
                                                    long long total, float* __restrict__ part) {
    __shared__ float sh[2][GT / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long stride = (long long)gridDim.x * GT;
    float lo = INFINITY, hi = -INFINITY;
    for (long long i0 = (long long)blockIdx.x * GT + t; i0 < total; i0 += MM_UNROLL * stride) {
        float v[MM_UNROLL];
#pragma unroll
        for (int u = 0; u < MM_UNROLL; ++u) {
            const long long i = i0 + u * stride;
            v[u] = i < total ? elem(x, s, C, H, W, i, dense) : NAN;  // (fminf / fmaxf pass over a NaN)
        }
#pragma unroll
        for (int u = 0; u < MM_UNROLL; ++u) {
            lo = fminf(lo, v[u]);
            hi = fmaxf(hi, v[u]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
        sh[0][wave] = lo;
        sh[1][wave] = hi;
    }
    __syncthreads();
    if (t == 0) {
        part[2 * blockIdx.x + 0] = fminf(fminf(sh[0][0], sh[0][1]), fminf(sh[0][2], sh[0][3]));
        part[2 * blockIdx.x + 1] = fmaxf(fmaxf(sh[1][0], sh[1][1]), fmaxf(sh[1][2], sh[1][3]));
    }
}

// save_image: mul(255).add_(0.5).clamp_(0, 255) and a truncating cast; a NaN gives 0 (fmaxf(NaN, 0) is 0)
__device__ __forceinline__ unsigned quantise(float v) {
    const float q = __fadd_rn(__fmul_rn(v, 255.f), 0.5f);
    return (unsigned)fminf(fmaxf(q, 0.f), 255.f);
}

// make_grid's norm_range: clamp, subtract the low end, DIVIDE by max(high - low, 1e-5)
__device__ __forceinline__ float normalise(float x, float lo, float hi, float div) {
    return __fdiv_rn(__fsub_rn(fminf(fmaxf(x, lo), hi), lo), div);
}

struct Geom {
    int n, c, h, w;
    int xmaps, padding;   // padding as laid out: 0 for n == 1 (make_grid returns a single image as it is)
    int H, W;             // the picture
    int row_bytes, words; // 3 W; aligned words a row can touch: (3 W + 3) / 4 + 1
};

__global__ __launch_bounds__(GT) void grid_u8_k(const float* __restrict__ x, Strides s, Geom g, float pad_value, int mode, float lo,
                                                float hi, const float* __restrict__ part, int nparts, uint8_t* __restrict__ out,
                                                unsigned out_low_bits) {
    if (mode == MOVAE_GRID_MINMAX) {
        __shared__ float sh[2][GT / 64];
        const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
        float a = INFINITY, b = -INFINITY;
        if (t < nparts) {  // nparts <= MM_BLOCKS == GT
            a = part[2 * t];
            b = part[2 * t + 1];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a = fminf(a, __shfl_xor(a, o, 64));
            b = fmaxf(b, __shfl_xor(b, o, 64));
        }
        if (lane == 0) {
            sh[0][wave] = a;
            sh[1][wave] = b;
        }
        __syncthreads();
        lo = fminf(fminf(sh[0][0], sh[0][1]), fminf(sh[0][2], sh[0][3]));
        hi = fmaxf(fmaxf(sh[1][0], sh[1][1]), fmaxf(sh[1][2], sh[1][3]));
    }
    const float div = fmaxf(__fsub_rn(hi, lo), 1e-5f);

    const long long id = (long long)blockIdx.x * GT + threadIdx.x;
    const long long r64 = id / g.words;
    if (r64 >= g.H) return;
    const int r = (int)r64, j = (int)(id - r64 * g.words);
    const long long row_off = (long long)r * g.row_bytes;
    // the row starts `mis` bytes into an aligned word: word j holds the row's bytes 4 j - mis .. 4 j - mis + 3
    const int mis = (int)((out_low_bits + (unsigned)(row_off & 3)) & 3u);
    const int b0 = 4 * j - mis;
    if (b0 >= g.row_bytes) return;

    // the grid row's image row, or the padding
    const int cell_h = g.h + g.padding, cell_w = g.w + g.padding;
    const int yy = r - g.padding;
    const int cy = yy >= 0 ? yy / cell_h : 0;
    const int iy = yy >= 0 ? yy - cy * cell_h : g.h;  // iy >= h: a padding row
    const unsigned pad_byte = quantise(pad_value);

    unsigned word = 0;
    bool full = b0 >= 0 && b0 + 4 <= g.row_bytes;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int b = b0 + u;
        if (b < 0 || b >= g.row_bytes) continue;
        const int px = b / 3, ch = b - 3 * px;
        unsigned byte = pad_byte;
        const int xx = px - g.padding;
        if (iy < g.h && xx >= 0) {
            const int cx = xx / cell_w, ix = xx - cx * cell_w;
            const long long k = (long long)cy * g.xmaps + cx;
            if (ix < g.w && k < g.n) {  // (cx < xmaps follows from px < W)
                const long long off = k * s.n + (g.c == 1 ? 0 : ch) * s.c + iy * s.h + ix * s.w;
                float v = x[off];
                if (mode != MOVAE_GRID_RAW) v = normalise(v, lo, hi, div);
                byte = quantise(v);
            }
        }
        if (full)
            word |= byte << (8 * u);
        else
            out[row_off + b] = (uint8_t)byte;
    }
    if (full) *reinterpret_cast<unsigned*>(out + row_off + b0) = word;
}

bool is_dense(Strides s, int n, int c, int h, int w) {
    long long st[4] = {s.n, s.c, s.h, s.w};
    long long sz[4] = {n, c, h, w};
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

int minmax_blocks(long long total) {
    const long long want = (total + (long long)GT * MM_UNROLL - 1) / ((long long)GT * MM_UNROLL);
    return (int)(want < 1 ? 1 : (want > MM_BLOCKS ? MM_BLOCKS : want));
}

constexpr size_t WS_BYTES = MOVAE_WS_HEADER_BYTES + (size_t)2 * MM_BLOCKS * sizeof(float);

}  // namespace

extern "C" size_t movae_image_grid_ws_bytes(int n, int c, int h, int w) {
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return 0;
    return WS_BYTES;
}

extern "C" int movae_image_grid_u8(const float* x, long long sn, long long sc, long long sh, long long sw, int n, int c, int h, int w,
                                   int nrow, int padding, float pad_value, int mode, float lo, float hi, uint8_t* out, void* ws,
                                   size_t ws_bytes, movae_stream_t stream) {
    MOVAE_CHECK_ARG(x && out, "movae_image_grid_u8: null pointer");
    MOVAE_CHECK_ARG(n > 0 && h > 0 && w > 0 && nrow > 0, "movae_image_grid_u8: n %d, h %d, w %d, nrow %d must be positive", n, h, w, nrow);
    MOVAE_CHECK_ARG(padding >= 0, "movae_image_grid_u8: padding %d", padding);
    MOVAE_CHECK_ARG(c == 1 || c == 3, "movae_image_grid_u8: %d channels (1 or 3)", c);
    MOVAE_CHECK_ARG(mode >= MOVAE_GRID_RAW && mode <= MOVAE_GRID_MINMAX, "movae_image_grid_u8: mode %d (0 .. 2)", mode);
    if (mode == MOVAE_GRID_RANGE) MOVAE_CHECK_ARG(hi >= lo, "movae_image_grid_u8: value range (%g, %g) is empty or not a number", lo, hi);
    if (mode == MOVAE_GRID_MINMAX) {
        MOVAE_CHECK_ARG(ws, "movae_image_grid_u8: null workspace");
        MOVAE_CHECK_ARG(ws_bytes >= WS_BYTES, "movae_image_grid_u8: workspace %zu bytes < %zu", ws_bytes, WS_BYTES);
    }
    Geom g;
    g.n = n, g.c = c, g.h = h, g.w = w;
    g.padding = n == 1 ? 0 : padding;
    g.xmaps = nrow < n ? nrow : n;
    const long long ymaps = ((long long)n + g.xmaps - 1) / g.xmaps;
    const long long H = ymaps * ((long long)h + g.padding) + g.padding, W = (long long)g.xmaps * ((long long)w + g.padding) + g.padding;
    MOVAE_CHECK_ARG(H <= 0x7fffffffLL && 3 * W + 8 <= 0x7fffffffLL, "movae_image_grid_u8: a %lld x %lld picture is above the int range", H, W);
    g.H = (int)H, g.W = (int)W;
    g.row_bytes = 3 * g.W;
    g.words = (g.row_bytes + 3) / 4 + 1;
    const long long blocks = (H * g.words + GT - 1) / GT;
    MOVAE_CHECK_ARG(blocks <= 0x7fffffffLL, "movae_image_grid_u8: %lld blocks are above the grid limit", blocks);
    const Strides s{sn, sc, sh, sw};
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* part = nullptr;
    int nparts = 0;
    if (mode == MOVAE_GRID_MINMAX) {
        part = reinterpret_cast<float*>(static_cast<char*>(ws) + MOVAE_WS_HEADER_BYTES);
        const long long total = (long long)n * c * h * w;
        nparts = minmax_blocks(total);
        hipLaunchKernelGGL(grid_minmax_k, dim3(nparts), dim3(GT), 0, st, x, s, (int)is_dense(s, n, c, h, w), c, h, w, total, part);
        MOVAE_CHECK_LAUNCH("grid_minmax_k");
    }
    hipLaunchKernelGGL(grid_u8_k, dim3((unsigned)blocks), dim3(GT), 0, st, x, s, g, pad_value, mode, lo, hi, part, nparts, out,
                       (unsigned)(reinterpret_cast<uintptr_t>(out) & 3));
    MOVAE_CHECK_LAUNCH("grid_u8_k");
    return MOVAE_OK;
}
