// Batch assembly from a device-resident uint8 image set (data.py: DeviceBatchLoader):
//
//   batch_u8     out[j][y][x][ch] = lut[ch][store[idx[j]][y][x'][ch]], x' = w - 1 - x for a flipped row, else x.  One launch gathers the
//                batch's rows, flips them, converts them through the table (ToTensor / Normalize, computed once on the host) and writes
//                the fp32 NHWC batch the first convolution reads.  Row i of the store is flipped iff bit 31 of word 0 of
//                philox4x32_10(counter = (i, epoch), key = seed) is set: a function of (seed, epoch, dataset index) only, never of the
//                batch or the position in it.  The table (c * 256 floats, 3 KB at most) is staged in LDS.  A thread of the fast path
//                (w % 4 == 0, store 4-byte aligned) owns 4 pixels of one line: it reads their c dwords (4 * c bytes; an image and a
//                group start at multiples of 4 * c bytes) and writes c 16-byte stores, consecutive threads consecutive 16 c bytes of
//                out; with a flip it reads the mirrored group and emits its pixels in reverse.  Any other w, or an unaligned store,
//                takes one thread per element.  No atomics, no workspace, no device globals.  Bytes: b h w c read + 4 b h w c written.
#include "common.h"

namespace {

struct BatchU8Args {
    const uint8_t* store;
    const int* idx;
    const float* lut;
    float* out;
    long long groups;  // fast path: b * h * (w / 4); scalar path: b * h * w * c
    int h, w;
    int flip;
    unsigned seed_lo, seed_hi, epoch_lo, epoch_hi;
};

__device__ __forceinline__ bool row_flipped(const BatchU8Args& a, int i) {
    unsigned r[4];
    philox4x32_10((unsigned)i, 0u /* high word of a non-negative int index */, a.epoch_lo, a.epoch_hi, a.seed_lo, a.seed_hi, r);
    return (r[0] >> 31) != 0;
}

template <int C, bool FAST>
__global__ __launch_bounds__(256) void batch_u8_k(BatchU8Args a) {
    __shared__ float slut[C * 256];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) slut[ch * 256 + threadIdx.x] = a.lut[ch * 256 + threadIdx.x];
    __syncthreads();
    const long long stride = (long long)gridDim.x * 256;
    const size_t image_bytes = (size_t)a.h * a.w * C;
    if (FAST) {
        const int gw = a.w >> 2;                    // groups of 4 pixels per line
        const long long gi = (long long)a.h * gw;  // ... per image
        for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < a.groups; g += stride) {
            const long long j = g / gi;
            const int r = (int)(g - j * gi), y = r / gw, gx = r - y * gw;
            const int i = a.idx[j];
            const bool fl = a.flip != 0 && row_flipped(a, i);
            const int sgx = fl ? gw - 1 - gx : gx;
            const uint32_t* src = reinterpret_cast<const uint32_t*>(a.store + (size_t)i * image_bytes + ((size_t)y * a.w + 4 * sgx) * C);
            uint32_t wd[C];
#pragma unroll
            for (int q = 0; q < C; ++q) wd[q] = src[q];
            float v[4 * C];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    // byte of the source group as it stands and mirrored: both positions are compile-time, the select is on the values
                    const int fb = p * C + ch, rb = (3 - p) * C + ch;
                    const unsigned f = (wd[fb >> 2] >> (8 * (fb & 3))) & 0xffu, m = (wd[rb >> 2] >> (8 * (rb & 3))) & 0xffu;
                    v[p * C + ch] = slut[ch * 256 + (fl ? m : f)];
                }
            f32x4* dst = reinterpret_cast<f32x4*>(a.out + (size_t)g * (4 * C));
#pragma unroll
            for (int q = 0; q < C; ++q) dst[q] = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
        }
    } else {
        const long long line = (long long)a.w * C, per_image = (long long)a.h * line;
        for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < a.groups; e += stride) {
            const long long j = e / per_image;
            const long long r = e - j * per_image;
            const int y = (int)(r / line), xc = (int)(r - (long long)y * line), x = xc / C, ch = xc - x * C;
            const int i = a.idx[j];
            const bool fl = a.flip != 0 && row_flipped(a, i);
            const int sx = fl ? a.w - 1 - x : x;
            a.out[e] = slut[ch * 256 + a.store[(size_t)i * image_bytes + ((size_t)y * a.w + sx) * C + ch]];
        }
    }
}

}  // namespace

int movae_batch_u8(const uint8_t* store, const int* idx, int b, int h, int w, int c, const float* lut, int flip,
                   unsigned long long seed, unsigned long long epoch, float* out, movae_stream_t stream) {
    MOVAE_CHECK_ARG(store && idx && lut && out, "movae_batch_u8: null pointer");
    MOVAE_CHECK_ARG(b > 0 && h > 0 && w > 0, "movae_batch_u8: b, h, w must be positive (got %d, %d, %d)", b, h, w);
    MOVAE_CHECK_ARG(c == 1 || c == 3, "movae_batch_u8: 1 or 3 channels (got %d)", c);
    MOVAE_CHECK_ARG(((uintptr_t)out & 15) == 0, "movae_batch_u8: out must be 16-byte aligned");
    const bool fast = w % 4 == 0 && ((uintptr_t)store & 3) == 0;
    BatchU8Args a;
    a.store = store, a.idx = idx, a.lut = lut, a.out = out;
    a.groups = fast ? (long long)b * h * (w / 4) : (long long)b * h * w * c;
    a.h = h, a.w = w, a.flip = flip;
    a.seed_lo = (unsigned)seed, a.seed_hi = (unsigned)(seed >> 32), a.epoch_lo = (unsigned)epoch, a.epoch_hi = (unsigned)(epoch >> 32);
    const long long want = (a.groups + 255) / 256;
    const dim3 grid((unsigned)(want < 2048 ? want : 2048));  // grid-stride past 2048 blocks
    hipStream_t st = (hipStream_t)stream;
    if (c == 3) {
        if (fast) batch_u8_k<3, true><<<grid, 256, 0, st>>>(a);
        else batch_u8_k<3, false><<<grid, 256, 0, st>>>(a);
    } else {
        if (fast) batch_u8_k<1, true><<<grid, 256, 0, st>>>(a);
        else batch_u8_k<1, false><<<grid, 256, 0, st>>>(a);
    }
    MOVAE_CHECK_LAUNCH("batch_u8");
    return MOVAE_OK;
}
