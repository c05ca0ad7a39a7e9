// Training-crop augmentation on device: crop + antialiased bicubic resize + flip + colour jitter +
// Gaussian blur + salt-and-pepper noise + ImageNet normalisation, and the dot-map targets.
//
// Reference (the reference runs all of this on CPU in DataLoader workers):
//   RandomResizedCrop / _crop / _resize   datasets/transforms.py:9-43,133-171
//       TF.resize(bicubic, antialias=True) = torch F.interpolate(mode="bicubic", antialias=True)
//   RandomHorizontalFlip                  datasets/transforms.py:174-187
//   ColorJitter (brightness/contrast/saturation/hue)      datasets/transforms.py:190-201
//   GaussianBlur(kernel_size, sigma=(0.1, 5.0))           datasets/transforms.py:217-223
//   PepperSaltNoise                       datasets/transforms.py:242-255
//   Normalize(ImageNet mean/std)          datasets/crowd.py:64,162
//   generate_density_map (sigma = None)   datasets/utils.py:11-28
//
// Launches per batch of crops (all crops of all images in each launch, RB-row blocks):
//   resize_h: rows of each crop window -> [3][crop_h][out_w] scratch (horizontal AA-bicubic taps)
//             (resize_h_raw: the same from stored uint8 HWC / CHW or f32 CHW sources, rows staged in LDS)
//   resize_v: scratch -> [3][out_h][out_w] output (vertical taps), horizontal flip on the store
//   gray_partial, pointwise, blur_v, blur_h: the per-crop op lists (see pointwise_kernel)
// Byte work (HBM/L2-bound): every thread owns output columns, so all loads/stores are row-contiguous.
#include "ebc_common.h"

namespace {

constexpr int RB = 4;          // rows per workgroup in the resize passes

// torch's antialias bicubic filter (a = -0.5), UpSampleKernel.cpp aa path
__device__ __forceinline__ float aa_cubic(float x) {
    constexpr float a = -0.5f;
    x = fabsf(x);
    if (x < 1.f) return ((a + 2.f) * x - (a + 3.f)) * x * x + 1.f;
    if (x < 2.f) return (((x - 5.f) * x + 8.f) * x - 4.f) * a;
    return 0.f;
}

// taps of output index i for an in_size -> out_size AA resize: first input index, count, 1/sum
struct Taps { int lo, n; float center, inv, norm; };
__device__ __forceinline__ Taps aa_taps(int i, int in_size, int out_size) {
    const float scale = (float)in_size / (float)out_size;
    const float support = scale >= 1.f ? 2.f * scale : 2.f;
    Taps t;
    t.inv = scale >= 1.f ? 1.f / scale : 1.f;
    t.center = scale * ((float)i + 0.5f);
    t.lo = max((int)(t.center - support + 0.5f), 0);
    const int hi = min((int)(t.center + support + 0.5f), in_size);
    t.n = hi - t.lo;
    float s = 0.f;
    for (int j = 0; j < t.n; ++j) s += aa_cubic(((float)(j + t.lo) - t.center + 0.5f) * t.inv);
    t.norm = s != 0.f ? 1.f / s : 0.f;
    return t;
}
__device__ __forceinline__ float tap_w(const Taps& t, int j) {
    return aa_cubic(((float)(j + t.lo) - t.center + 0.5f) * t.inv) * t.norm;
}

__global__ __launch_bounds__(256) void resize_h_kernel(const float* __restrict__ src, const EbcCropDesc* __restrict__ desc,
                                                       float* __restrict__ ws)
{
    const EbcCropDesc d = desc[blockIdx.y / 3];
    const int c = blockIdx.y % 3, r0 = blockIdx.x * RB;
    if (r0 >= d.crop_h) return;
    const float* plane = src + d.src_off + (size_t)c * d.src_h * d.src_w;
    float* tmp = ws + d.tmp_off + (size_t)c * d.crop_h * d.out_w;
    for (int ox = threadIdx.x; ox < d.out_w; ox += blockDim.x) {
        const Taps t = aa_taps(ox, d.crop_w, d.out_w);
        for (int r = r0; r < min(r0 + RB, d.crop_h); ++r) {
            const float* row = plane + (size_t)(d.top + r) * d.src_w + d.left + t.lo;
            float acc = 0.f;
            for (int j = 0; j < t.n; ++j) acc = fmaf(tap_w(t, j), row[j], acc);
            tmp[(size_t)r * d.out_w + ox] = acc;
        }
    }
}

// ---- the horizontal pass from stored images (uint8 HWC / CHW, f32 CHW): resize_h_kernel's arithmetic, the source
// rows staged in LDS.  A workgroup owns RB rows of one crop (of one plane; of all three for HWC, whose bytes are
// interleaved) and one chunk of output columns whose input span fits a staged row.
constexpr int RAW_ROW_BYTES = 4096;                    // span bytes of one staged row
constexpr int RAW_LDW = RAW_ROW_BYTES / 4 + 1;         // + the up to 3 bytes in front of an unaligned row start
// RB rows of RAW_LDW dwords + the 256-entry u/255 table = 17.0 KiB: nine workgroups a CU by LDS, eight by waves

__host__ __device__ inline int raw_cap_px(int layout) {
    return layout == EBC_EVAL_U8_HWC ? RAW_ROW_BYTES / 3 : layout == EBC_EVAL_U8_CHW ? RAW_ROW_BYTES : RAW_ROW_BYTES / 4;
}
// output columns per chunk.  With S = ceil(crop_w / out_w) >= scale the input span of oc columns is at most
// scale (oc - 1) + 2 support + 1 + rounding <= S oc + 3 S + 2 pixels (support <= 2 S), which this keeps <= the cap;
// integer arithmetic, so the host's grid and the kernel agree
__host__ __device__ inline int raw_chunk_cols(int layout, int crop_w, int out_w) {
    const int S = (crop_w + out_w - 1) / out_w;
    const int oc = (raw_cap_px(layout) - 2 - 4 * S) / S;
    return oc < 1 ? 1 : (oc > out_w ? out_w : oc);
}

template <int LAYOUT>
__device__ __forceinline__ void resize_h_raw_body(const uint8_t* __restrict__ src, const EbcCropSrc& s, const EbcCropDesc& d,
                                                  int c, int r0, int chunk, float* __restrict__ ws,
                                                  uint32_t (*lds)[RAW_LDW], const float* lut)
{
    constexpr bool F32 = LAYOUT == EBC_EVAL_F32_CHW;
    constexpr int NC = LAYOUT == EBC_EVAL_U8_HWC ? 3 : 1;          // channels a workgroup owns = bytes per pixel step
    const int tid = threadIdx.x;
    const int oc = raw_chunk_cols(LAYOUT, d.crop_w, d.out_w);
    const int ox0 = chunk * oc;
    if (ox0 >= d.out_w) return;
    const int ox1 = min(ox0 + oc, d.out_w);
    const Taps tf = aa_taps(ox0, d.crop_w, d.out_w), tl = aa_taps(ox1 - 1, d.crop_w, d.out_w);
    const int lo0 = tf.lo, span = tl.lo + tl.n - lo0;              // input columns [lo0, lo0 + span) of the window
    // a single column's taps wider than a staged row (a > 250-fold reduction): read the source directly
    const bool staged = span <= raw_cap_px(LAYOUT);
    const int nr = min(RB, d.crop_h - r0);
    const uint8_t* row[RB];                                        // first needed byte of each row
    int sh[RB];                                                    // its offset from the aligned dword below it
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const int y = d.top + r0 + min(r, nr - 1);
        const size_t px = LAYOUT == EBC_EVAL_U8_HWC ? ((size_t)y * s.W + d.left + lo0) * 3
                                                    : ((size_t)c * s.H + y) * s.W + d.left + lo0;
        row[r] = src + s.src_off + px * (F32 ? 4 : 1);
        sh[r] = F32 ? 0 : (int)(reinterpret_cast<uintptr_t>(row[r]) & 3);
    }
    if (staged) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            if (r >= nr) continue;
            if (F32) {
                const uint32_t* g = reinterpret_cast<const uint32_t*>(row[r]);
                for (int i = tid; i < span; i += 256) lds[r][i] = g[i];
            } else {
                // bytes [s0, end) relative to the aligned address a0: single bytes up to the first dword boundary b0,
                // whole dwords to the last boundary b1, single bytes after it
                const int s0 = sh[r], end = s0 + span * NC;
                const int b0 = (s0 + 3) & ~3, b1 = end & ~3;
                const uint8_t* a0 = row[r] - s0;                   // (never dereferenced below row[r])
                const uint32_t* g = reinterpret_cast<const uint32_t*>(a0);
                uint8_t* l = reinterpret_cast<uint8_t*>(lds[r]);
                for (int i = (b0 >> 2) + tid; i < (b1 >> 2); i += 256) lds[r][i] = g[i];
                const int he = min(b0, end), tb = max(b1, b0);
                if (s0 + tid < he) l[s0 + tid] = a0[s0 + tid];
                if (tb + tid < end) l[tb + tid] = a0[tb + tid];
            }
        }
        __syncthreads();
    }
    for (int ox = ox0 + tid; ox < ox1; ox += 256) {
        const Taps t = aa_taps(ox, d.crop_w, d.out_w);
        const int rel = t.lo - lo0;
        float acc[RB][NC];
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) acc[r][cc] = 0.f;
        for (int j = 0; j < t.n; ++j) {
            const float w = tap_w(t, j);
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                if (r >= nr) continue;
#pragma unroll
                for (int cc = 0; cc < NC; ++cc) {
                    float px;
                    if (F32) {
                        px = staged ? __uint_as_float(lds[r][rel + j]) : reinterpret_cast<const float*>(row[r])[rel + j];
                    } else {
                        const int b = (rel + j) * NC + cc;
                        px = lut[staged ? reinterpret_cast<const uint8_t*>(lds[r])[sh[r] + b] : row[r][b]];
                    }
                    acc[r][cc] = fmaf(w, px, acc[r][cc]);
                }
            }
        }
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            float* tmp = ws + d.tmp_off + (size_t)(c + cc) * d.crop_h * d.out_w;
#pragma unroll
            for (int r = 0; r < RB; ++r)
                if (r < nr) tmp[(size_t)(r0 + r) * d.out_w + ox] = acc[r][cc];
        }
    }
}

// grid (row blocks of the tallest crop, 3 n, column chunks of the crop with the most)
__global__ __launch_bounds__(256) void resize_h_raw_kernel(const uint8_t* __restrict__ src, const EbcCropSrc* __restrict__ csrc,
                                                           const EbcCropDesc* __restrict__ desc, float* __restrict__ ws)
{
    __shared__ uint32_t lds[RB][RAW_LDW];
    __shared__ float lut[256];
    const int k = blockIdx.y / 3, c = blockIdx.y % 3, r0 = blockIdx.x * RB;
    const EbcCropSrc s = csrc[k];
    const EbcCropDesc d = desc[k];
    if (r0 >= d.crop_h || (s.layout == EBC_EVAL_U8_HWC && c != 0)) return;
    lut[threadIdx.x] = (float)threadIdx.x / 255.0f;                // the conversion, one correctly rounded division each
    __syncthreads();
    if (s.layout == EBC_EVAL_U8_HWC) resize_h_raw_body<EBC_EVAL_U8_HWC>(src, s, d, 0, r0, blockIdx.z, ws, lds, lut);
    else if (s.layout == EBC_EVAL_U8_CHW) resize_h_raw_body<EBC_EVAL_U8_CHW>(src, s, d, c, r0, blockIdx.z, ws, lds, lut);
    else resize_h_raw_body<EBC_EVAL_F32_CHW>(src, s, d, c, r0, blockIdx.z, ws, lds, lut);
}

__global__ __launch_bounds__(256) void resize_v_kernel(const EbcCropDesc* __restrict__ desc, const float* __restrict__ ws,
                                                       float* __restrict__ out)
{
    const EbcCropDesc d = desc[blockIdx.y / 3];
    const int c = blockIdx.y % 3, y0 = blockIdx.x * RB;
    if (y0 >= d.out_h) return;
    const float* tmp = ws + d.tmp_off + (size_t)c * d.crop_h * d.out_w;
    float* o = out + d.out_off + (size_t)c * d.out_h * d.out_w;
    for (int y = y0; y < min(y0 + RB, d.out_h); ++y) {
        const Taps t = aa_taps(y, d.crop_h, d.out_h);
        for (int ox = threadIdx.x; ox < d.out_w; ox += blockDim.x) {
            float acc = 0.f;
            for (int j = 0; j < t.n; ++j) acc = fmaf(tap_w(t, j), tmp[(size_t)(t.lo + j) * d.out_w + ox], acc);
            o[(size_t)y * d.out_w + (d.flip ? d.out_w - 1 - ox : ox)] = acc;
        }
    }
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
// TF.rgb_to_grayscale for float images: 0.2989 r + 0.587 g + 0.114 b
__device__ __forceinline__ float gray(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }

// counter-based uniform [0, 1): murmur3 finaliser of (seed, element index), 24 random bits
__device__ __forceinline__ float hash_uniform(uint32_t seed, uint32_t idx) {
    uint32_t h = seed ^ (idx * 0x9E3779B9u);
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// The per-crop op list, spread over many workgroups per crop (a single CU per crop is bound by the
// bytes one CU keeps in flight): rows are cut into RB-row blocks, every pass is its own launch.
//   gray_partial : crops with a contrast op -- per-block grey sums of the image as it stands before
//                  that op (the earlier jitter ops applied on the fly), into the crop's scratch
//   pointwise    : all jitter ops (contrast's mean = the fixed-order sum of those partials); crops
//                  without blur also get noise + normalisation here
//   blur_v/blur_h: GaussianBlur (vertical taps into scratch, horizontal taps + noise + normalisation)
struct Pix { float r, g, b; };

// torchvision F.adjust_hue on one float pixel, in its float32 operations (_rgb2hsv, h = (h + f) % 1, _hsv2rgb; the
// reference's masks select exactly one term, so the masked sums are that term); no contraction into FMAs, so each
// operation rounds as the reference's separate tensor ops do
__device__ __forceinline__ Pix adjust_hue(Pix px, float hf) {
#pragma clang fp contract(off)
    const float r = px.r, g = px.g, b = px.b;
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.0f : maxc);
    const float crd = eqc ? 1.0f : cr;
    const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
    float h;
    if (maxc == r) h = bc - gc;
    else if (maxc == g) h = (2.0f + rc) - bc;
    else h = (4.0f + gc) - rc;
    h = fmodf(h / 6.0f + 1.0f, 1.0f);
    // (h + hue) % 1.0: torch.remainder (fmod, then + 1 for a negative remainder)
    float hh = fmodf(h + hf, 1.0f);
    if (hh != 0.0f && hh < 0.0f) hh += 1.0f;
    const float v = maxc;
    const float fi = floorf(hh * 6.0f);
    const float f = hh * 6.0f - fi;
    int i = (int)fi % 6;
    if (i < 0) i += 6;
    const float p = fminf(fmaxf(v * (1.0f - s), 0.0f), 1.0f);
    const float q = fminf(fmaxf(v * (1.0f - s * f), 0.0f), 1.0f);
    const float t = fminf(fmaxf(v * (1.0f - s * (1.0f - f)), 0.0f), 1.0f);
    switch (i) {
        case 0: return {v, t, p};
        case 1: return {q, v, p};
        case 2: return {p, v, t};
        case 3: return {p, q, v};
        case 4: return {t, p, v};
        default: return {v, p, q};
    }
}

__device__ __forceinline__ Pix jitter_apply(Pix p, int ops, int from, int to, const EbcCropDesc& d, float cmean) {
    for (int slot = from; slot < to; ++slot) {
        const int op = (ops >> (3 * slot)) & 7;
        if (op == 1) {
            p.r = clamp01(d.brightness * p.r); p.g = clamp01(d.brightness * p.g); p.b = clamp01(d.brightness * p.b);
        } else if (op == 2) {
            const float f = d.contrast, mb = (1.f - f) * cmean;
            p.r = clamp01(f * p.r + mb); p.g = clamp01(f * p.g + mb); p.b = clamp01(f * p.b + mb);
        } else if (op == 3) {
            const float f = d.saturation, gm = (1.f - f) * gray(p.r, p.g, p.b);
            p.r = clamp01(f * p.r + gm); p.g = clamp01(f * p.g + gm); p.b = clamp01(f * p.b + gm);
        } else if (op == 4) {
            p = adjust_hue(p, d.hue);
        }
    }
    return p;
}

__device__ __forceinline__ float finish_px(float v, int c, int e, const EbcCropDesc& d, const float* __restrict__ noise,
                                          const EbcAugConst& k) {
    if (d.noise) {
        const float u = d.noise_off >= 0 && noise ? noise[d.noise_off + e] : hash_uniform(d.seed, (uint32_t)e);
        if (u < d.saltiness) v = 1.f;
        if (u > 1.f - d.spiciness) v = 0.f;
    }
    if (d.normalize) v = (v - k.mean[c]) / k.std[c];
    return v;
}

__device__ __forceinline__ int n_ops(int ops) { int n = 0; while (n < 4 && ((ops >> (3 * n)) & 7)) ++n; return n; }
__device__ __forceinline__ int contrast_slot(int ops) {
    int c = -1;
    for (int s = 0; s < 4; ++s) if (((ops >> (3 * s)) & 7) == 2) c = s;
    return c;
}

constexpr int PT = 256;        // pointwise / blur threads

__device__ float block_sum_pt(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(PT) void gray_partial_kernel(const EbcCropDesc* __restrict__ desc, const float* __restrict__ out,
                                                         float* __restrict__ ws)
{
    __shared__ float red[PT / 64];
    const EbcCropDesc d = desc[blockIdx.y];
    const int cs = contrast_slot(d.jitter_ops), y0 = blockIdx.x * RB;
    if (cs < 0 || y0 >= d.out_h) return;
    const int HW = d.out_h * d.out_w;
    const float* R = out + d.out_off;
    float s = 0.f;
    for (int y = y0; y < min(y0 + RB, d.out_h); ++y)
        for (int x = threadIdx.x; x < d.out_w; x += PT) {
            const int e = y * d.out_w + x;
            const Pix p = jitter_apply({R[e], R[HW + e], R[2 * HW + e]}, d.jitter_ops, 0, cs, d, 0.f);
            s += gray(p.r, p.g, p.b);
        }
    s = block_sum_pt(s, red);
    if (threadIdx.x == 0) ws[d.tmp_off + blockIdx.x] = s;
}

__global__ __launch_bounds__(PT) void pointwise_kernel(const EbcCropDesc* __restrict__ desc, float* __restrict__ out,
                                                      const float* __restrict__ ws, const float* __restrict__ noise,
                                                      EbcAugConst k)
{
    const EbcCropDesc d = desc[blockIdx.y];
    const int y0 = blockIdx.x * RB, nops = n_ops(d.jitter_ops);
    if (y0 >= d.out_h || (nops == 0 && d.blur) || (nops == 0 && !d.noise && !d.normalize)) return;
    float cmean = 0.f;
    if (contrast_slot(d.jitter_ops) >= 0) {
        const int nb = (d.out_h + RB - 1) / RB;
        for (int i = 0; i < nb; ++i) cmean += ws[d.tmp_off + i];       // fixed order: reproducible
        cmean /= (float)(d.out_h * d.out_w);
    }
    const int HW = d.out_h * d.out_w;
    float* R = out + d.out_off;
    for (int y = y0; y < min(y0 + RB, d.out_h); ++y)
        for (int x = threadIdx.x; x < d.out_w; x += PT) {
            const int e = y * d.out_w + x;
            Pix p = jitter_apply({R[e], R[HW + e], R[2 * HW + e]}, d.jitter_ops, 0, nops, d, cmean);
            if (!d.blur) {
                p.r = finish_px(p.r, 0, e, d, noise, k);
                p.g = finish_px(p.g, 1, HW + e, d, noise, k);
                p.b = finish_px(p.b, 2, 2 * HW + e, d, noise, k);
            }
            R[e] = p.r; R[HW + e] = p.g; R[2 * HW + e] = p.b;
        }
}

// normalised pdf over linspace(-(ks-1)/2, (ks-1)/2, ks) (torchvision _get_gaussian_kernel1d)
__device__ void blur_taps(float* kk, int ks, float sigma) {
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < ks; ++i) {
            const float x = (float)i - 0.5f * (float)(ks - 1);
            kk[i] = expf(-0.5f * (x / sigma) * (x / sigma));
            s += kk[i];
        }
        for (int i = 0; i < ks; ++i) kk[i] /= s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(PT) void blur_v_kernel(const EbcCropDesc* __restrict__ desc, const float* __restrict__ out,
                                                   float* __restrict__ ws, EbcAugConst k)
{
    __shared__ float ky[EBC_AUG_MAX_BLUR];
    const EbcCropDesc d = desc[blockIdx.y / 3];
    const int c = blockIdx.y % 3, y0 = blockIdx.x * RB, H = d.out_h, W = d.out_w, hk = k.blur_k / 2;
    if (!d.blur || y0 >= H) return;
    blur_taps(ky, k.blur_k, k.sigma_y);
    const float* P = out + d.out_off + (size_t)c * H * W;
    float* S = ws + d.tmp_off + (size_t)c * H * W;
    for (int y = y0; y < min(y0 + RB, H); ++y)
        for (int x = threadIdx.x; x < W; x += PT) {
            float acc = 0.f;
            for (int i = 0; i < k.blur_k; ++i) acc = fmaf(ky[i], P[reflect(y + i - hk, H) * W + x], acc);
            S[y * W + x] = acc;
        }
}

__global__ __launch_bounds__(PT) void blur_h_kernel(const EbcCropDesc* __restrict__ desc, float* __restrict__ out,
                                                   const float* __restrict__ ws, const float* __restrict__ noise,
                                                   EbcAugConst k)
{
    __shared__ float kx[EBC_AUG_MAX_BLUR];
    const EbcCropDesc d = desc[blockIdx.y / 3];
    const int c = blockIdx.y % 3, y0 = blockIdx.x * RB, H = d.out_h, W = d.out_w, hk = k.blur_k / 2;
    if (!d.blur || y0 >= H) return;
    blur_taps(kx, k.blur_k, k.sigma_x);
    const float* S = ws + d.tmp_off + (size_t)c * H * W;
    float* O = out + d.out_off + (size_t)c * H * W;
    for (int y = y0; y < min(y0 + RB, H); ++y)
        for (int x = threadIdx.x; x < W; x += PT) {
            float acc = 0.f;
            for (int i = 0; i < k.blur_k; ++i) acc = fmaf(kx[i], S[y * W + reflect(x + i - hk, W)], acc);
            O[y * W + x] = finish_px(acc, c, c * H * W + y * W + x, d, noise, k);
        }
}

// dot map: out[b][0][clamp(int y)][clamp(int x)] = 1 (zeroed by the launcher)
__global__ void point_map_kernel(const float* __restrict__ pts, const int* __restrict__ offsets, int B, int H, int W,
                                 float* __restrict__ out)
{
    const int b = blockIdx.y;
    const int p0 = offsets[b], n = offsets[b + 1] - p0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int x = min(max((int)pts[2 * (p0 + i)], 0), W - 1);
        const int y = min(max((int)pts[2 * (p0 + i) + 1], 0), H - 1);
        out[((size_t)b * H + y) * W + x] = 1.0f;
    }
}

}  // namespace

// the per-crop op lists on the resized crops: gray_partial, pointwise, blur_v, blur_h
static int launch_crop_ops(const EbcCropDesc* desc, int n, int max_out_h, float* out, float* workspace, const float* noise,
                           EbcAugConst k, hipStream_t st)
{
    const int nb = (max_out_h + RB - 1) / RB;
    hipLaunchKernelGGL(gray_partial_kernel, dim3(nb, n), dim3(PT), 0, st, desc, out, workspace);
    EBC_CHECK_LAUNCH();
    hipLaunchKernelGGL(pointwise_kernel, dim3(nb, n), dim3(PT), 0, st, desc, out, workspace, noise, k);
    EBC_CHECK_LAUNCH();
    hipLaunchKernelGGL(blur_v_kernel, dim3(nb, 3 * n), dim3(PT), 0, st, desc, out, workspace, k);
    EBC_CHECK_LAUNCH();
    hipLaunchKernelGGL(blur_h_kernel, dim3(nb, 3 * n), dim3(PT), 0, st, desc, out, workspace, noise, k);
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

extern "C" int ebc_augment_crops(const float* src, const EbcCropDesc* desc, int n, int max_crop_h, int max_out_h,
                                 float* out, float* workspace, const float* noise, EbcAugConst k, ebc_stream_t stream)
{
    if (n < 0 || !desc || !out || !workspace || max_crop_h < 0 || max_out_h < 0) return EBC_E_ARG;
    if (k.blur_k < 1 || k.blur_k > EBC_AUG_MAX_BLUR || (k.blur_k & 1) == 0) return EBC_E_ARG;
    if (n == 0) return EBC_OK;
    hipStream_t st = (hipStream_t)stream;
    if (src && max_crop_h > 0) {
        hipLaunchKernelGGL(resize_h_kernel, dim3((max_crop_h + RB - 1) / RB, 3 * n), dim3(256), 0, st, src, desc, workspace);
        EBC_CHECK_LAUNCH();
        hipLaunchKernelGGL(resize_v_kernel, dim3((max_out_h + RB - 1) / RB, 3 * n), dim3(256), 0, st, desc, workspace, out);
        EBC_CHECK_LAUNCH();
    }
    return launch_crop_ops(desc, n, max_out_h, out, workspace, noise, k, st);
}

extern "C" int ebc_augment_crops_raw(const void* src, const EbcCropSrc* csrc, const EbcCropSrc* csrc_host,
                                     const EbcCropDesc* desc, const EbcCropDesc* desc_host, int n, float* out,
                                     float* workspace, const float* noise, EbcAugConst k, ebc_stream_t stream)
{
    constexpr long long I32 = 0x7FFFFFFFll;
    if (!src || !csrc || !csrc_host || !desc || !desc_host || !out || !workspace || n < 0 || 3ll * n > 65535) return EBC_E_ARG;
    if (k.blur_k < 1 || k.blur_k > EBC_AUG_MAX_BLUR || (k.blur_k & 1) == 0) return EBC_E_ARG;
    int max_crop_h = 0, max_out_h = 0, max_chunks = 1;
    for (int i = 0; i < n; ++i) {
        const EbcCropSrc& s = csrc_host[i];
        const EbcCropDesc& d = desc_host[i];
        if (s.layout != EBC_EVAL_U8_HWC && s.layout != EBC_EVAL_U8_CHW && s.layout != EBC_EVAL_F32_CHW) return EBC_E_ARG;
        if (s.src_off < 0 || s.H <= 0 || s.W <= 0 || 3ll * s.H * s.W > I32) return EBC_E_ARG;
        if (s.layout == EBC_EVAL_F32_CHW && ((s.src_off & 3) || (reinterpret_cast<uintptr_t>(src) & 3))) return EBC_E_ARG;
        if (d.crop_h <= 0 || d.crop_w <= 0 || d.out_h <= 0 || d.out_w <= 0 || d.top < 0 || d.left < 0) return EBC_E_ARG;
        if ((long long)d.top + d.crop_h > s.H || (long long)d.left + d.crop_w > s.W) return EBC_E_ARG;
        if (3ll * d.crop_h * d.out_w > I32 || 3ll * d.out_h * d.out_w > I32) return EBC_E_ARG;
        const int oc = raw_chunk_cols(s.layout, d.crop_w, d.out_w), chunks = (d.out_w + oc - 1) / oc;
        if (chunks > 65535) return EBC_E_ARG;
        max_crop_h = d.crop_h > max_crop_h ? d.crop_h : max_crop_h;
        max_out_h = d.out_h > max_out_h ? d.out_h : max_out_h;
        max_chunks = chunks > max_chunks ? chunks : max_chunks;
    }
    if (n == 0) return EBC_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(resize_h_raw_kernel, dim3((max_crop_h + RB - 1) / RB, 3 * n, max_chunks), dim3(256), 0, st,
                       (const uint8_t*)src, csrc, desc, workspace);
    EBC_CHECK_LAUNCH();
    hipLaunchKernelGGL(resize_v_kernel, dim3((max_out_h + RB - 1) / RB, 3 * n), dim3(256), 0, st, desc, workspace, out);
    EBC_CHECK_LAUNCH();
    return launch_crop_ops(desc, n, max_out_h, out, workspace, noise, k, st);
}

extern "C" int ebc_point_map(const float* points, const int* offsets, int B, int H, int W, int max_points, float* out,
                             ebc_stream_t stream)
{
    if (B < 0 || H <= 0 || W <= 0 || !out || (B > 0 && !offsets)) return EBC_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, sizeof(float) * (size_t)B * H * W, st) != hipSuccess) return EBC_E_LAUNCH;
    if (B == 0 || max_points <= 0) return EBC_OK;
    hipLaunchKernelGGL(point_map_kernel, dim3((max_points + 255) / 256, B), dim3(256), 0, st, points, offsets, B, H, W, out);
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}
