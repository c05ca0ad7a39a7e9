// Evaluation of a split from raw images: tile gather straight from uint8 sources (convert, zero-pad, normalise
// and tile in one pass), uint8 -> f32 [0, 1] for the resize branch, and the overlap-averaged assembly of a whole
// batch of images with their counts.
//
// Reference (val split, all on CPU there): datasets/crowd.py:141-162 (`/255.`, Normalize), datasets/transforms.py:
// 69-134 (Resize2Multiple / ZeroPad2Multiple), utils/eval_utils.py:26-96 (tiling and assembly), eval.py:27 (count).
//
// The tile list is global: image i owns tiles tile0 .. tile0 + rows*cols, so one model batch may span images.
// Byte work, HBM-bound: a thread owns four consecutive x of one tile row (all three channels), loads the aligned
// dwords that cover its source bytes and stores one float4 per channel; consecutive lanes take consecutive x.
// All index math is 32-bit (sizes are checked on the host), one 32-bit division per thread.
#include "ebc_common.h"

namespace {

__device__ __forceinline__ int tile_start(int i, int stride, int win, int full) {
    const int s = i * stride;
    return (s + win > full) ? full - win : s;
}

struct Norm { float mean[3], std[3]; };

// (u / 255 - mean) / std in the reference's three f32 operations (crowd.py:144,162), each rounded on its own
__device__ __forceinline__ float norm_u8(uint32_t u, float mean, float std) {
#pragma clang fp contract(off)
    const float a = (float)u / 255.0f;
    const float b = a - mean;
    return b / std;
}
__device__ __forceinline__ float norm_pad(float mean, float std) {
#pragma clang fp contract(off)
    const float b = 0.0f - mean;
    return b / std;
}

// the image that owns global tile t (tile0 ascending; block-uniform, so the loads are scalar)
__device__ __forceinline__ int owner(const EbcEvalImage* __restrict__ desc, int n, int t) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[mid].tile0 <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// bytes [a, a + nbytes) of src (nbytes <= 12, > 0) as three dwords starting at byte a: only the aligned dwords that
// hold one of those bytes are loaded, so nothing outside the dwords of the image's own bytes is touched (src itself
// is dword-aligned; a is the offset from it, so an image may start at any byte)
__device__ __forceinline__ void load_span(const uint8_t* __restrict__ src, size_t a, int nbytes, uint32_t out[3]) {
    const size_t a0 = a & ~(size_t)3;
    const int sh = (int)(a - a0), last = sh + nbytes - 1;          // last needed byte, relative to a0 (<= 14)
    const uint32_t* p = reinterpret_cast<const uint32_t*>(src + a0);
    uint32_t w[4];
    w[0] = p[0];
    w[1] = last >= 4 ? p[1] : 0u;
    w[2] = last >= 8 ? p[2] : 0u;
    w[3] = last >= 12 ? p[3] : 0u;
    const int s8 = 8 * sh;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (uint32_t)((((uint64_t)w[k + 1] << 32) | w[k]) >> s8);
}

// tiles [nt][3][wh][ww] f32 <- tiles t0 .. t0 + nt of the global list.  grid (nt, ceil(wh * ww/4 / 256))
__global__ __launch_bounds__(256) void tiles_from_raw_kernel(const uint8_t* __restrict__ src,
                                                             const EbcEvalImage* __restrict__ desc, int n_images, int wh,
                                                             int ww, int sh, int sw, int t0, Norm k,
                                                             float* __restrict__ tiles)
{
    const int ww4 = ww >> 2;
    const int u = blockIdx.y * 256 + threadIdx.x;
    if (u >= wh * ww4) return;
    const int y = u / ww4, x = (u - y * ww4) << 2;
    const int t = t0 + blockIdx.x;
    const EbcEvalImage d = desc[owner(desc, n_images, t)];
    const int tl = t - d.tile0, ti = tl / d.cols, tj = tl - ti * d.cols;
    const int sy = tile_start(ti, sh, wh, d.Hf) + y, sx = tile_start(tj, sw, ww, d.Wf) + x;
    const int nv = sy < d.H ? min(max(d.W - sx, 0), 4) : 0;        // pixels of this thread inside the stored image
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float pad = norm_pad(k.mean[c], k.std[c]);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[c][i] = pad;
    }
    if (nv > 0) {
        if (d.layout == EBC_EVAL_U8_HWC) {
            uint32_t w[3];
            load_span(src, (size_t)d.src_off + (size_t)((sy * d.W + sx) * 3), 3 * nv, w);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int b = 3 * i + c;
                    if (i < nv) v[c][i] = norm_u8((w[b >> 2] >> (8 * (b & 3))) & 0xFFu, k.mean[c], k.std[c]);
                }
        } else if (d.layout == EBC_EVAL_U8_CHW) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                uint32_t w[3];
                load_span(src, (size_t)d.src_off + (size_t)((c * d.H + sy) * d.W + sx), nv, w);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < nv) v[c][i] = norm_u8((w[0] >> (8 * i)) & 0xFFu, k.mean[c], k.std[c]);
            }
        } else {                                                   // f32 CHW, already normalised
            const float* f = reinterpret_cast<const float*>(src + d.src_off);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* row = f + (c * d.H + sy) * d.W + sx;
                if (nv == 4 && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {
                    const float4 q = *reinterpret_cast<const float4*>(row);
                    v[c][0] = q.x; v[c][1] = q.y; v[c][2] = q.z; v[c][3] = q.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (i < nv) v[c][i] = row[i];
                }
            }
        }
    }
    float* o = tiles + ((int)blockIdx.x * 3 * wh + y) * ww + x;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(o + c * wh * ww) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
}

// out [3][H][W] f32 = u8 / 255.  A thread owns four consecutive elements of a plane.
__global__ __launch_bounds__(256) void u8_to_chw01_kernel(const uint8_t* __restrict__ src, int layout, int HW,
                                                          float* __restrict__ out)
{
    const int p = (blockIdx.x * 256 + threadIdx.x) << 2;
    const int nv = min(HW - p, 4);
    if (nv <= 0) return;
    if (layout == EBC_EVAL_U8_HWC && blockIdx.y != 0) return;
    auto store = [&](int c, const float* vc) {
        float* o = out + c * HW + p;
        if (nv == 4 && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
            *reinterpret_cast<float4*>(o) = make_float4(vc[0], vc[1], vc[2], vc[3]);
        } else {
            for (int i = 0; i < nv; ++i) o[i] = vc[i];
        }
    };
    uint32_t w[3];
    if (layout == EBC_EVAL_U8_HWC) {
        float v[3][4];
        load_span(src, (size_t)p * 3, 3 * nv, w);                  // 12 p is dword-aligned: three plain loads
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int b = 3 * i + c;
                v[c][i] = (float)((w[b >> 2] >> (8 * (b & 3))) & 0xFFu) / 255.0f;
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) store(c, v[c]);
    } else {
        const int c = blockIdx.y;
        float v[4];
        load_span(src, (size_t)(c * HW + p), nv, w);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (float)((w[0] >> (8 * i)) & 0xFFu) / 255.0f;
        store(c, v);
    }
}

// maps + map_off [Cp][Hf/r][Wf/r] of image blockIdx.y = mean over its covering tiles of preds [T][Cp][wh/r][ww/r]
// (tile_assemble_kernel's arithmetic: the sum runs over the tile rows, then the tile columns, then one division)
__global__ __launch_bounds__(256) void assemble_batch_kernel(const float* __restrict__ preds,
                                                             const EbcEvalImage* __restrict__ desc, int Cp, int wh, int ww,
                                                             int sh, int sw, int r, float* __restrict__ maps)
{
    const EbcEvalImage d = desc[blockIdx.y];
    const int Ho = d.Hf / r, Wo = d.Wf / r, ph = wh / r, pw = ww / r;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Cp * Ho * Wo) return;
    const int c = e / (Ho * Wo), q = e - c * Ho * Wo, y = q / Wo, x = q - y * Wo;
    float s = 0.f, n = 0.f;
    for (int i = 0; i < d.rows; ++i) {
        const int ts = tile_start(i, sh, wh, d.Hf), ys = ts / r, ye = (ts + wh) / r;
        if (y < ys || y >= ye) continue;
        for (int j = 0; j < d.cols; ++j) {
            const int us = tile_start(j, sw, ww, d.Wf), xs = us / r, xe = (us + ww) / r;
            if (x < xs || x >= xe) continue;
            s += preds[(((d.tile0 + i * d.cols + j) * Cp + c) * ph + (y - ys)) * pw + (x - xs)];
            n += 1.f;
        }
    }
    maps[d.map_off + e] = s / n;
}

// counts[i] = sum of image i's map, one workgroup an image, in a fixed order (no atomics: two launches give the same
// bits): thread t adds elements t, t + 1024, ... into four rotating partials, then a binary tree over the 4096
// partials.  A term passes through at most ceil(n / 4096) + 12 additions (44 for the 2^17 elements of a 2048 x 3072
// image at reduction 8 with Cp = 1).
constexpr int CT = 1024;
__global__ __launch_bounds__(CT) void map_count_kernel(const EbcEvalImage* __restrict__ desc, int Cp, int r,
                                                      const float* __restrict__ maps, float* __restrict__ counts)
{
    __shared__ float red[CT];
    const EbcEvalImage d = desc[blockIdx.x];
    const int n = Cp * (d.Hf / r) * (d.Wf / r);
    const float* m = maps + d.map_off;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    int e = threadIdx.x;
    for (; e + 3 * CT < n; e += 4 * CT) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += m[e + k * CT];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (e + k * CT < n) a[k] += m[e + k * CT];
    red[threadIdx.x] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    for (int o = CT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = red[0];
}

constexpr long long I32 = 0x7FFFFFFFll;

// What both batch entry points require of the descriptors (read from the host copy): returns the total tile count,
// or -1.  Every product the kernels form in 32 bits is bounded here.
long long check_images(const EbcEvalImage* h, int n, int wh, int ww, int sh, int sw)
{
    if (!h || n <= 0 || wh <= 0 || ww <= 0 || sh <= 0 || sw <= 0 || sh > wh || sw > ww) return -1;
    long long tiles = 0;
    for (int i = 0; i < n; ++i) {
        const EbcEvalImage& d = h[i];
        if (d.layout != EBC_EVAL_U8_HWC && d.layout != EBC_EVAL_U8_CHW && d.layout != EBC_EVAL_F32_CHW) return -1;
        if (d.H <= 0 || d.W <= 0 || d.Hf < d.H || d.Wf < d.W || d.Hf < wh || d.Wf < ww) return -1;
        if (d.src_off < 0 || d.map_off < 0) return -1;
        if (d.layout == EBC_EVAL_F32_CHW && (d.src_off & 3)) return -1;
        if (3ll * d.Hf * d.Wf > I32) return -1;                    // covers 3 H W and every row/column product
        const long long rows = ((long long)d.Hf - wh + sh - 1) / sh + 1, cols = ((long long)d.Wf - ww + sw - 1) / sw + 1;
        if (d.rows != rows || d.cols != cols || d.tile0 != tiles) return -1;
        tiles += rows * cols;
        if (tiles > I32) return -1;
    }
    return tiles;
}

}  // namespace

extern "C" int ebc_tiles_from_raw(const void* src, const EbcEvalImage* desc, const EbcEvalImage* desc_host, int n_images,
                                  int wh, int ww, int sh, int sw, int tile_begin, int tile_count, const float* mean,
                                  const float* std, float* tiles, ebc_stream_t stream)
{
    if (!src || !desc || !tiles || !mean || !std || (ww & 3)) return EBC_E_ARG;
    if ((reinterpret_cast<uintptr_t>(src) & 3) || (reinterpret_cast<uintptr_t>(tiles) & 15)) return EBC_E_ARG;
    const long long total = check_images(desc_host, n_images, wh, ww, sh, sw);
    if (total < 0 || tile_begin < 0 || tile_count < 0 || (long long)tile_begin + tile_count > total) return EBC_E_ARG;
    if (3ll * wh * ww * tile_count > I32 || (long long)wh * (ww >> 2) > 65535ll * 256) return EBC_E_ARG;
    if (tile_count == 0) return EBC_OK;
    Norm k;
    for (int c = 0; c < 3; ++c) { k.mean[c] = mean[c]; k.std[c] = std[c]; }
    const int units = wh * (ww >> 2);
    hipLaunchKernelGGL(tiles_from_raw_kernel, dim3(tile_count, (units + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)src, desc, n_images, wh, ww, sh, sw, tile_begin, k, tiles);
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

extern "C" int ebc_u8_to_chw01(const void* src, int layout, int H, int W, float* out, ebc_stream_t stream)
{
    if (!src || !out || H <= 0 || W <= 0 || (layout != EBC_EVAL_U8_HWC && layout != EBC_EVAL_U8_CHW)) return EBC_E_ARG;
    if ((reinterpret_cast<uintptr_t>(src) & 3) || (reinterpret_cast<uintptr_t>(out) & 3)) return EBC_E_ARG;
    if (3ll * H * W > I32) return EBC_E_ARG;
    const int HW = H * W, nb = ((HW + 3) / 4 + 255) / 256;
    hipLaunchKernelGGL(u8_to_chw01_kernel, dim3(nb, layout == EBC_EVAL_U8_HWC ? 1 : 3), dim3(256), 0,
                       (hipStream_t)stream, (const uint8_t*)src, layout, HW, out);
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

extern "C" int ebc_tiles_assemble_batch(const float* preds, const EbcEvalImage* desc, const EbcEvalImage* desc_host,
                                        int n_images, int Cp, int wh, int ww, int sh, int sw, int reduction, float* maps,
                                        float* counts, ebc_stream_t stream)
{
    if (!preds || !desc || !maps || !counts || Cp <= 0 || reduction <= 0) return EBC_E_ARG;
    const long long total = check_images(desc_host, n_images, wh, ww, sh, sw);
    if (total < 0 || n_images > 65535) return EBC_E_ARG;
    if (total * Cp * (wh / reduction) * (ww / reduction) > I32) return EBC_E_ARG;
    long long biggest = 0;
    for (int i = 0; i < n_images; ++i) {
        const long long n = (long long)Cp * (desc_host[i].Hf / reduction) * (desc_host[i].Wf / reduction);
        if (n <= 0 || n > I32 || desc_host[i].map_off + n > I32) return EBC_E_ARG;
        biggest = n > biggest ? n : biggest;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(assemble_batch_kernel, dim3((unsigned)((biggest + 255) / 256), n_images), dim3(256), 0, st, preds,
                       desc, Cp, wh, ww, sh, sw, reduction, maps);
    EBC_CHECK_LAUNCH();
    hipLaunchKernelGGL(map_count_kernel, dim3(n_images), dim3(CT), 0, st, desc, Cp, reduction, maps, counts);
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}
