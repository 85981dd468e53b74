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
//   batch_u8_staged  the same kernel body for a STREAMED set (data.py: StreamedBatchLoader): the batch's rows were gathered on the host
//                and copied into a device staging buffer in batch order, so the source row of out[j] is stage[j] while the flip is
//                still keyed by the dataset index ids[j].  The same (seed, epoch, index) gives the same pixels as batch_u8.
//   batch_rrc_u8 the same for a RAGGED set (data.py: RaggedBatchLoader): images of their own sizes back to back in one blob, and per
//                image a crop box that is resampled to s x s exactly as PIL's crop(box).resize((s, s), BICUBIC) does it, then mirrored
//                and sent through the table.  One launch, a block per 32 x 32 output tile; described at the kernel below.
//   resample_coeffs  the coefficient-table routine of batch_rrc_u8 alone, for many input sizes in one launch (a test entry).
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

// STAGED: the source row of out[j] is store[j] (a staging buffer in batch order) and idx[j] only keys the flip; otherwise store[idx[j]].
template <int C, bool FAST, bool STAGED>
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
            const size_t row = STAGED ? (size_t)j : (size_t)i;
            const uint32_t* src = reinterpret_cast<const uint32_t*>(a.store + row * image_bytes + ((size_t)y * a.w + 4 * sgx) * C);
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
            const size_t row = STAGED ? (size_t)j : (size_t)i;
            a.out[e] = slut[ch * 256 + a.store[row * image_bytes + ((size_t)y * a.w + sx) * C + ch]];
        }
    }
}

// ---- batch_rrc_u8: RandomResizedCrop batches from a ragged set ----------------------------------------------------------------------
// PIL's 8-bit resample, which is what the reference's RandomResizedCrop(BICUBIC) runs on its PIL images, is integer arithmetic behind
// a coefficient table: per output position a window of taps [xmin, xmin + n) and n weights, Keys' cubic (a = -0.5) at
// (tap - center + 0.5) * (1 / filterscale) -- a product with the reciprocal, as in PIL's C --, each divided by their sum in fp64 and
// fixed to 22 fractional bits.  A pass is clip8((2^21 + sum pixel * k) >> 22) in int32 (8 + 22 + 2 bits); the horizontal pass comes
// first and is ROUNDED TO BYTES before the vertical one.  coeff_row restates the table in fp64 with contraction off (a fused
// multiply-add moves a weight by a unit in the last place), one IEEE division per weight (by the sum) and the tap-order sum, so the
// device reproduces PIL bit for bit.

constexpr int RRC_TILE = 32;    // output tile side of one block
constexpr int RRC_KMAX = 33;    // taps at filterscale 8: 2 * ceil(2 * 8) + 1
constexpr int RRC_SPAN = 288;   // crop rows / columns under one tile: <= 31 * 8 + 2 * 16 + 1 = 281
constexpr int RRC_STAGE = 8;    // crop rows staged per step of the horizontal pass
constexpr double RRC_ONE = 4194304.0;  // 2^22

__device__ __forceinline__ double keys_cubic(double x) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Output position o of an axis resampled from `in` to `out` samples: bounds = (first tap, taps n), k[0 .. kmax) = the fixed-point
// weights (zero from n on).  n is cut at kmax, so k is never overrun whatever `in` is.
__device__ void coeff_row(int in, int out, int o, int kmax, int* k, int* bounds) {
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    const double center = (o + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    int n = xmax - xmin;
    n = n < 0 ? 0 : (n > kmax ? kmax : n);
    double ww = 0.0;
    for (int t = 0; t < n; ++t) ww += keys_cubic(((double)(t + xmin) - center + 0.5) * ss);
    for (int t = 0; t < kmax; ++t) {
        int v = 0;
        if (t < n) {  // the weight again, not a stored copy: no per-thread array
            double w = keys_cubic(((double)(t + xmin) - center + 0.5) * ss);
            if (ww != 0.0) w = w / ww;
            v = w < 0 ? (int)(-0.5 + w * RRC_ONE) : (int)(0.5 + w * RRC_ONE);
        }
        k[t] = v;
    }
    bounds[0] = xmin, bounds[1] = n;
}

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> 22;  // arithmetic
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct RrcArgs {
    const uint8_t* blob;
    const long long* offsets;
    const int* dims;
    const int* boxes;
    const int* idx;
    const float* lut;
    float* out;
    int s, kmax, flip;
    unsigned seed_lo, seed_hi, epoch_lo, epoch_hi;
};

// One block: one RRC_TILE x RRC_TILE output tile of one image.  Tables of the tile's columns and lines -> horizontal pass over the crop
// rows the tile's lines tap, RRC_STAGE rows at a time through a byte-granular staging buffer (an image starts at any byte), into the
// uint8 tile sh[row][x][ch] -> vertical pass, value table, store (mirrored along x for a flipped image).  LDS, C = 3: 46.6 KB.
template <int C>
__global__ __launch_bounds__(256) void batch_rrc_k(RrcArgs a) {
    __shared__ float slut[C * 256];
    __shared__ int skx[RRC_TILE * RRC_KMAX], sky[RRC_TILE * RRC_KMAX], sbx[RRC_TILE * 2], sby[RRC_TILE * 2];
    __shared__ uint8_t sh[RRC_SPAN * RRC_TILE * C];
    __shared__ uint8_t sseg[RRC_STAGE * RRC_SPAN * C];
    const int tid = threadIdx.x, s = a.s;
    const int tiles = (s + RRC_TILE - 1) / RRC_TILE;
    const int j = blockIdx.x / (tiles * tiles), tile = blockIdx.x - j * tiles * tiles;
    const int y0 = (tile / tiles) * RRC_TILE, x0 = (tile % tiles) * RRC_TILE;
    const int tw = s - x0 < RRC_TILE ? s - x0 : RRC_TILE, th = s - y0 < RRC_TILE ? s - y0 : RRC_TILE;
    const int i = a.idx[j];
    const int width = a.dims[2 * i + 1];
    const int top = a.boxes[4 * i], left = a.boxes[4 * i + 1], bh = a.boxes[4 * i + 2], bw = a.boxes[4 * i + 3];
    const uint8_t* img = a.blob + a.offsets[i];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) slut[ch * 256 + tid] = a.lut[ch * 256 + tid];
    if ((tid & 3) == 0) {  // 64 table rows, 16 per wave
        const int r = tid >> 2, o = r & (RRC_TILE - 1);
        if (r < RRC_TILE) {
            if (o < tw) coeff_row(bw, s, x0 + o, a.kmax, skx + o * RRC_KMAX, sbx + 2 * o);
        } else if (o < th) {
            coeff_row(bh, s, y0 + o, a.kmax, sky + o * RRC_KMAX, sby + 2 * o);
        }
    }
    __syncthreads();
    const int r0 = sby[0], c0 = sbx[0];
    int nrows = sby[2 * (th - 1)] + sby[2 * (th - 1) + 1] - r0, ncols = sbx[2 * (tw - 1)] + sbx[2 * (tw - 1) + 1] - c0;
    // The caller keeps every crop side <= 8 s and kmax at the set's true bound; then neither count is cut.  A call that breaks either
    // stays inside LDS and inside the image through these cuts (and coeff_row's), but its pixels are undefined, not an error.
    nrows = nrows > RRC_SPAN ? RRC_SPAN : nrows, ncols = ncols > RRC_SPAN ? RRC_SPAN : ncols;
    const int segb = ncols * C;
    const int lx = tid & (RRC_TILE - 1), lr = tid >> 5;
    for (int rb = 0; rb < nrows; rb += RRC_STAGE) {
        const int nr = nrows - rb < RRC_STAGE ? nrows - rb : RRC_STAGE;
        for (int e = tid; e < nr * segb; e += 256) {
            const int rr = e / segb, off = e - rr * segb;
            sseg[rr * (RRC_SPAN * C) + off] = img[((size_t)(top + r0 + rb + rr) * width + left + c0) * C + off];
        }
        __syncthreads();
        if (lr < nr && lx < tw) {
            const int xm = sbx[2 * lx] - c0;
            int n = sbx[2 * lx + 1];
            if (xm + n > ncols) n = ncols - xm;
            const uint8_t* p = sseg + lr * (RRC_SPAN * C) + xm * C;
            const int* k = skx + lx * RRC_KMAX;
            int acc[C];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[ch] = 1 << 21;
            for (int t = 0; t < n; ++t) {
                const int kv = k[t];
#pragma unroll
                for (int ch = 0; ch < C; ++ch) acc[ch] += (int)p[t * C + ch] * kv;
            }
#pragma unroll
            for (int ch = 0; ch < C; ++ch) sh[((rb + lr) * RRC_TILE + lx) * C + ch] = (uint8_t)clip8(acc[ch]);
        }
        __syncthreads();
    }
    bool fl = false;
    if (a.flip != 0) {
        unsigned r[4];
        philox4x32_10((unsigned)i, 0u /* stream 0: the flip's */, a.epoch_lo, a.epoch_hi, a.seed_lo, a.seed_hi, r);
        fl = (r[0] >> 31) != 0;
    }
    const int xd0 = fl ? s - x0 - tw : x0;  // the tile's first column in out: the flip mirrors the OUTPUT columns
    const int rowf = tw * C;
    float* obase = a.out + (size_t)j * s * s * C;
    auto value = [&](int y, int f) -> float {  // float f of line y of the tile as it lies in out
        const int xd = f / C, ch = f - xd * C, x = fl ? tw - 1 - xd : xd;
        const int ym = sby[2 * y] - r0;
        int n = sby[2 * y + 1];
        if (ym + n > nrows) n = nrows - ym;
        int acc = 1 << 21;
        for (int t = 0; t < n; ++t) acc += (int)sh[((ym + t) * RRC_TILE + x) * C + ch] * sky[y * RRC_KMAX + t];
        return slut[ch * 256 + clip8(acc)];
    };
    // consecutive threads, consecutive 16-byte pieces: with s * C a multiple of 4 every tile row is whole aligned pieces (x0 is a
    // multiple of 32, tw is 32 or s % 32, xd0 is x0 or s - x0 - tw: all times C are multiples of 4 then)
    if (((s * C) & 3) == 0) {
        const int q = rowf >> 2;
        for (int e = tid; e < th * q; e += 256) {
            const int y = e / q, p = e - y * q;
            const f32x4 v = {value(y, 4 * p), value(y, 4 * p + 1), value(y, 4 * p + 2), value(y, 4 * p + 3)};
            *reinterpret_cast<f32x4*>(obase + ((size_t)(y0 + y) * s + xd0) * C + 4 * p) = v;
        }
    } else {
        for (int e = tid; e < th * rowf; e += 256) {
            const int y = e / rowf, f = e - y * rowf;
            obase[((size_t)(y0 + y) * s + xd0) * C + f] = value(y, f);
        }
    }
}

__global__ __launch_bounds__(256) void resample_coeffs_k(const int* in_sizes, long long rows, int out, int kmax, int* k, int* bounds) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows) return;
    coeff_row(in_sizes[e / out], out, (int)(e % out), kmax, k + e * kmax, bounds + 2 * e);
}

}  // namespace

int movae_batch_rrc_u8(const uint8_t* blob, const long long* offsets, const int* dims, const int* boxes, const int* idx, int b, int s, int c,
                       int kmax, const float* lut, int flip, unsigned long long seed, unsigned long long epoch, float* out,
                       movae_stream_t stream) {
    MOVAE_CHECK_ARG(blob && offsets && dims && boxes && idx && lut && out, "movae_batch_rrc_u8: null pointer");
    MOVAE_CHECK_ARG(b > 0 && s > 0, "movae_batch_rrc_u8: b and s must be positive (got %d, %d)", b, s);
    MOVAE_CHECK_ARG(c == 1 || c == 3, "movae_batch_rrc_u8: 1 or 3 channels (got %d)", c);
    MOVAE_CHECK_ARG(kmax >= 5 && kmax <= RRC_KMAX && (kmax & 1), "movae_batch_rrc_u8: kmax is odd, 5 .. %d (got %d)", RRC_KMAX, kmax);
    MOVAE_CHECK_ARG(((uintptr_t)out & 15) == 0, "movae_batch_rrc_u8: out must be 16-byte aligned");
    const long long tiles = (s + RRC_TILE - 1) / RRC_TILE, blocks = tiles * tiles * b;
    MOVAE_CHECK_ARG(blocks <= 0x7fffffffLL, "movae_batch_rrc_u8: %lld tiles are more than one grid", blocks);
    RrcArgs a;
    a.blob = blob, a.offsets = offsets, a.dims = dims, a.boxes = boxes, a.idx = idx, a.lut = lut, a.out = out;
    a.s = s, a.kmax = kmax, a.flip = flip;
    a.seed_lo = (unsigned)seed, a.seed_hi = (unsigned)(seed >> 32), a.epoch_lo = (unsigned)epoch, a.epoch_hi = (unsigned)(epoch >> 32);
    hipStream_t st = (hipStream_t)stream;
    if (c == 3) batch_rrc_k<3><<<dim3((unsigned)blocks), 256, 0, st>>>(a);
    else batch_rrc_k<1><<<dim3((unsigned)blocks), 256, 0, st>>>(a);
    MOVAE_CHECK_LAUNCH("batch_rrc_u8");
    return MOVAE_OK;
}

int movae_resample_coeffs(const int* in_sizes, int n, int out_size, int kmax, int* k, int* bounds, movae_stream_t stream) {
    MOVAE_CHECK_ARG(in_sizes && k && bounds, "movae_resample_coeffs: null pointer");
    MOVAE_CHECK_ARG(n > 0 && out_size > 0, "movae_resample_coeffs: n and out_size must be positive (got %d, %d)", n, out_size);
    MOVAE_CHECK_ARG(kmax >= 5 && (kmax & 1), "movae_resample_coeffs: kmax is odd and at least 5 (got %d)", kmax);
    const long long rows = (long long)n * out_size;
    MOVAE_CHECK_ARG(rows * kmax <= 0x7fffffffLL, "movae_resample_coeffs: %lld table entries are more than one call's", rows * kmax);
    resample_coeffs_k<<<dim3((unsigned)((rows + 255) / 256)), 256, 0, (hipStream_t)stream>>>(in_sizes, rows, out_size, kmax, k, bounds);
    MOVAE_CHECK_LAUNCH("resample_coeffs");
    return MOVAE_OK;
}

// movae_batch_u8 and movae_batch_u8_staged: the same checks and the same launch, `name` in the messages
template <bool STAGED>
static int batch_u8_launch(const char* name, const uint8_t* store, const int* idx, int b, int h, int w, int c, const float* lut, int flip,
                           unsigned long long seed, unsigned long long epoch, float* out, movae_stream_t stream) {
    MOVAE_CHECK_ARG(store && idx && lut && out, "%s: null pointer", name);
    MOVAE_CHECK_ARG(b > 0 && h > 0 && w > 0, "%s: b, h, w must be positive (got %d, %d, %d)", name, b, h, w);
    MOVAE_CHECK_ARG(c == 1 || c == 3, "%s: 1 or 3 channels (got %d)", name, c);
    MOVAE_CHECK_ARG(((uintptr_t)out & 15) == 0, "%s: out must be 16-byte aligned", name);
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
        if (fast) batch_u8_k<3, true, STAGED><<<grid, 256, 0, st>>>(a);
        else batch_u8_k<3, false, STAGED><<<grid, 256, 0, st>>>(a);
    } else {
        if (fast) batch_u8_k<1, true, STAGED><<<grid, 256, 0, st>>>(a);
        else batch_u8_k<1, false, STAGED><<<grid, 256, 0, st>>>(a);
    }
    MOVAE_CHECK_LAUNCH(name);
    return MOVAE_OK;
}

int movae_batch_u8(const uint8_t* store, const int* idx, int b, int h, int w, int c, const float* lut, int flip,
                   unsigned long long seed, unsigned long long epoch, float* out, movae_stream_t stream) {
    return batch_u8_launch<false>("movae_batch_u8", store, idx, b, h, w, c, lut, flip, seed, epoch, out, stream);
}

int movae_batch_u8_staged(const uint8_t* stage, const int* ids, int b, int h, int w, int c, const float* lut, int flip,
                          unsigned long long seed, unsigned long long epoch, float* out, movae_stream_t stream) {
    return batch_u8_launch<true>("movae_batch_u8_staged", stage, ids, b, h, w, c, lut, flip, seed, epoch, out, stream);
}
