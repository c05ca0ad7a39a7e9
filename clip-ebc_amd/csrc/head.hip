// The blockwise image-text similarity head on gfx950: forward, backward (d Z, d bias, d logit_scale) and the gradient
// of the raw text rows (freeze_text_encoder=False), with their C-ABI entry points.
//
// Reference: similarity head              models/clip/model.py:198-217
//
// Why the kernels below repeat pieces of each other.  They sit at the register limit, and sharing device code between
// them moved the compiler's choices (this file at the Makefile's flags plus --cuda-device-only -S, compared per kernel;
// NOTHING WAS TIMED -- the register and instruction counts alone kept both out):
//   * The tail of head_text_bwd_kernel / head_text_wide_bwd_kernel (the wave-order combine into red / pblk; the two
//     copies are byte-identical) as one __forceinline__ function: head_text_bwd_kernel<float, 512> went from
//     next_free_vgpr 255 to 434 (accum_offset 256: 178 AGPRs used as spill space), the f16 / bf16 instances from 243 to
//     428, the 1024-wide instances from 244 to 254.  Passing w and lane in changed nothing.
//   * A four-line pix_norm<NV>(v) (sum of squares, wave_sum, sqrtf) at the four sites that spell it out: every
//     head_bwd_kernel<..., 1024, ...> instance changed -- CAP 16: 226 -> 254 VGPRs (f32 Z), 170 -> 206 (16-bit Z),
//     4441 -> 5617 instructions; CAP 32, 16-bit Z: 208 -> 238.  The forward instances changed order, not size.
// So the device code stays as it is, and only the host side below is shared.
#include <type_traits>

#include "ebc_common.h"
#include "kernels.h"
#include "mfma.h"
#include "vec_io.h"

using namespace ebc;

namespace {

// ----------------------------------------------------------------------------- similarity head
// One wave per pixel, CH channels (CH / 64 per lane, in float4 pieces 256 apart), NB <= CAP bins (CAP = the capacity of
// the per-pixel register arrays: 16, or 32 = EBC_HEAD_MAX_BINS for 17 .. 32 bins; the launchers pick the instance by
// NB, so a call with NB <= 16 runs the CAP = 16 instance it always ran); the text
// features are normalised in LDS.  CH = 512 (ViT-B/16) or 1024 (ResNet-50, models/clip/model.py:85-95).
// pixels per 4-wave block (r02, tools/kbench.py head): the forward is fastest with one pixel per wave (4: 15.7 us vs
// 18.5 at 16, 16 crops); the backward with 8 per wave (32: 38.2 vs 42.2 us; fewer blocks also mean fewer d bias
// partial rows for head_bias_finalize_kernel to sum)
constexpr int HEAD_FWD_PPB = 4, HEAD_BWD_PPB = 32;

template <class TZ, int CH>
__device__ __forceinline__ void load_pix(const TZ* z, float (&v)[CH / 64]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < CH / 256; ++q) {
        const float4 a = ld4<TZ>(z + 256 * q + 4 * lane);
        v[4 * q] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
    }
}

template <int CH>
__device__ void load_text(const float* text, int NB, float* tn) {
    // tn[k][c] = text[k][c] / max(||text[k]||, 1e-12)   (F.normalize, model.py:204): each text row read once, as
    // float4 pieces held in registers across the norm (the per-element loop re-read it, 2 x CH/64 dependent loads)
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    for (int k = w; k < NB; k += blockDim.x / 64) {
        float4 x[CH / 256];
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < CH / 256; ++q) {
            x[q] = *reinterpret_cast<const float4*>(text + k * CH + 256 * q + 4 * lane);
            s += (x[q].x * x[q].x + x[q].y * x[q].y) + (x[q].z * x[q].z + x[q].w * x[q].w);
        }
        s = wave_sum(s);
        const float inv = 1.0f / fmaxf(sqrtf(s), 1e-12f);
#pragma unroll
        for (int q = 0; q < CH / 256; ++q)
            *reinterpret_cast<float4*>(tn + k * CH + 256 * q + 4 * lane) =
                make_float4(x[q].x * inv, x[q].y * inv, x[q].z * inv, x[q].w * inv);
    }
    __syncthreads();
}

// <scaled pixel, normalised text row> partial of this lane (its CH / 64 channels)
template <int CH>
__device__ __forceinline__ float text_dot(const float* t, const float* zs) {
    const int lane = threadIdx.x & 63;
    float d = 0.f;
#pragma unroll
    for (int q = 0; q < CH / 256; ++q) {
        const float4 a = *reinterpret_cast<const float4*>(t + 256 * q + 4 * lane);
        d += zs[4 * q] * a.x + zs[4 * q + 1] * a.y + zs[4 * q + 2] * a.z + zs[4 * q + 3] * a.w;
    }
    return d;
}

template <class TZ, int CH, int CAP = 16>
__global__ __launch_bounds__(256) void head_fwd_kernel(const TZ* __restrict__ Z, const float* text, const float* logit_scale,
                                                       const float* anchors, float* logits, float* expo, int P, int HW, int NB)
{
    constexpr int NV = CH / 64;
    extern __shared__ __attribute__((aligned(16))) float tn[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    constexpr int PPW = HEAD_FWD_PPB / 4;            // pixels per wave: every row load issued up front,
    float vv[PPW][NV];                                // before the text normalisation (latencies overlap)
#pragma unroll
    for (int j = 0; j < PPW; ++j) load_pix<TZ, CH>(Z + (size_t)min(blockIdx.x * HEAD_FWD_PPB + w + 4 * j, P - 1) * CH, vv[j]);
    const float s = expf(*logit_scale);
    load_text<CH>(text, NB, tn);
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        const int p = blockIdx.x * HEAD_FWD_PPB + w + 4 * j;
        if (p >= P) break;
        float* v = vv[j];
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) ss += v[j] * v[j];
        const float inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
        float zs[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) zs[j] = s * (v[j] * inv);
        float lg[CAP];
        float mx = -INFINITY;
        for (int k = 0; k < NB; ++k) {
            lg[k] = wave_sum(text_dot<CH>(tn + k * CH, zs));
            mx = fmaxf(mx, lg[k]);
        }
        float se = 0.f;
        for (int k = 0; k < NB; ++k) se += expf(lg[k] - mx);
        float e = 0.f;
        for (int k = 0; k < NB; ++k) e += (expf(lg[k] - mx) / se) * anchors[k];
        if (lane == 0) {
            const int b = p / HW, hw = p % HW;
            for (int k = 0; k < NB; ++k) logits[((size_t)b * NB + k) * HW + hw] = lg[k];
            expo[(size_t)b * HW + hw] = e;
        }
    }
}

// dZ = d/dZ of (logits, exp) given upstream dlogits [B,NB,HW], dexp [B,1,HW] (x *gscale if given);
// also this block's d bias (column sums of its dZ rows) and d logit_scale partial: part[block][0..CH) and
// part[block][CH] (plain stores; head_bias_finalize_kernel sums the blocks in order -- bit-reproducible, where float
// atomics from every block into the same CH addresses were neither reproducible nor free of contention).
template <class TZ, class TD, int CH, int CAP = 16>
__global__ __launch_bounds__(256) void head_bwd_kernel(const TZ* __restrict__ Z, const float* text, const float* logit_scale,
                                                       const float* anchors, const float* dlogits, const float* dexp,
                                                       const float* gscale, TD* dZ, float* part, int P, int HW, int NB)
{
    constexpr int NV = CH / 64;
    extern __shared__ __attribute__((aligned(16))) float tn[];
    float* dbias_l = tn + NB * CH;       // [4 waves][CH]
    float* dsc_l = dbias_l + 4 * CH;     // [4]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    constexpr int PPW = HEAD_BWD_PPB / 4;            // pixels per wave: every row load issued up front,
    float vv[PPW][NV];                                // before the text normalisation (latencies overlap)
#pragma unroll
    for (int j = 0; j < PPW; ++j) load_pix<TZ, CH>(Z + (size_t)min(blockIdx.x * HEAD_BWD_PPB + w + 4 * j, P - 1) * CH, vv[j]);
    const float ls = *logit_scale, s = expf(ls);
    const float gs = gscale ? *gscale : 1.0f;
    load_text<CH>(text, NB, tn);
    float db[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) db[j] = 0.f;
    float dsc = 0.f;
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        const int p = blockIdx.x * HEAD_BWD_PPB + w + 4 * j;
        if (p >= P) break;
        float* v = vv[j];
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) ss += v[j] * v[j];
        const float nrm = sqrtf(wave_sum(ss));
        const float den = fmaxf(nrm, 1e-12f), inv = 1.0f / den;
        float zn[NV], zs[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) { zn[j] = v[j] * inv; zs[j] = s * zn[j]; }
        float lg[CAP], pr[CAP];
        float mx = -INFINITY;
        for (int k = 0; k < NB; ++k) {
            lg[k] = wave_sum(text_dot<CH>(tn + k * CH, zs));
            mx = fmaxf(mx, lg[k]);
        }
        float se = 0.f;
        for (int k = 0; k < NB; ++k) { pr[k] = expf(lg[k] - mx); se += pr[k]; }
        float e = 0.f;
        for (int k = 0; k < NB; ++k) { pr[k] /= se; e += pr[k] * anchors[k]; }
        const int b = p / HW, hw = p % HW;
        const float de = dexp[(size_t)b * HW + hw] * gs;
        float dzn[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) dzn[j] = 0.f;
        for (int k = 0; k < NB; ++k) {
            // d logit_k = dlogits_k + dexp * p_k (anchor_k - e)   (softmax + expectation backward)
            const float dl = dlogits[((size_t)b * NB + k) * HW + hw] * gs + de * pr[k] * (anchors[k] - e);
            dsc += dl * lg[k];                             // logits = exp(ls) * cos  ->  d ls = dl * logits
            const float* t = tn + k * CH;
            const float c = dl * s;
#pragma unroll
            for (int q = 0; q < NV / 4; ++q) {
                const float4 a = *reinterpret_cast<const float4*>(t + 256 * q + 4 * lane);
                dzn[4 * q] += c * a.x; dzn[4 * q + 1] += c * a.y; dzn[4 * q + 2] += c * a.z; dzn[4 * q + 3] += c * a.w;
            }
        }
        // F.normalize backward: dz = (dzn - zn * <zn, dzn>) / ||z||   (or dzn / eps when clamped)
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) dot += zn[j] * dzn[j];
        dot = (nrm > 1e-12f) ? wave_sum(dot) : 0.f;
        float dz[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) { dz[j] = (dzn[j] - zn[j] * dot) * inv; db[j] += dz[j]; }
#pragma unroll
        for (int q = 0; q < NV / 4; ++q)
            st4<TD>(dZ + (size_t)p * CH + 256 * q + 4 * lane, make_float4(dz[4 * q], dz[4 * q + 1], dz[4 * q + 2], dz[4 * q + 3]));
    }
    // lane 0's dsc is the wave's per-pixel sum (wave_sum results are lane-uniform)
#pragma unroll
    for (int q = 0; q < NV / 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) dbias_l[w * CH + 256 * q + 4 * lane + j] = db[4 * q + j];
    if (lane == 0) dsc_l[w] = dsc;
    __syncthreads();
    if (!part) return;
    float* pr = part + (size_t)blockIdx.x * (CH + 1);
    for (int c = threadIdx.x; c < CH; c += blockDim.x)
        pr[c] = (dbias_l[c] + dbias_l[CH + c]) + (dbias_l[2 * CH + c] + dbias_l[3 * CH + c]);
    if (threadIdx.x == 0) pr[CH] = (dsc_l[0] + dsc_l[1]) + (dsc_l[2] + dsc_l[3]);
}

// dbias[c] = sum over blocks of part[b][c] (c < CH), dscale = sum of part[b][CH], blocks in order
// 64 columns per workgroup, 8 waves: wave w sums blocks w, w + 8, ... in eight interleaved chains (all eight loads
// of a round in flight: one serial chain of nblk dependent L2 round trips per lane took 31 us per step at 392 blocks),
// then the 8 wave sums are combined in wave order -- a fixed order, so the result is bit-reproducible
template <int CH>
__global__ __launch_bounds__(512) void head_bias_finalize_kernel(const float* __restrict__ part, int nblk, float* dbias,
                                                                 float* dscale)
{
    __shared__ float ws[8][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const bool live = c <= CH;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int b = w;
    for (; b + 56 < nblk; b += 64) {
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] += live ? part[(size_t)(b + 8 * j) * (CH + 1) + c] : 0.f;
    }
    for (int j = 0; b < nblk; b += 8, ++j) s[j & 7] += live ? part[(size_t)b * (CH + 1) + c] : 0.f;
    ws[w][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    __syncthreads();
    if (w == 0 && live) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += ws[k][lane];
        if (c < CH) { if (dbias) dbias[c] = t; }
        else if (dscale) *dscale = t;
    }
}

// ---- d text (freeze_text_encoder=False, models/clip/model.py:201-208): the gradient of (logits, exp) with respect to
// the RAW text rows, through the head's own F.normalize of them.  With dl[p][k] as head_bwd_kernel forms it,
//   dtn_k = exp(ls) sum_p dl[p][k] zn_p,   <tn_k, dtn_k> = sum_p dl[p][k] logits[p][k]   (logits = exp(ls) <zn, tn>)
//   dt_k  = (dtn_k - tn_k <tn_k, dtn_k>) / max(||t_k||, 1e-12)       (dtn_k / 1e-12 where the norm is clamped)
// A kernel of its own that recomputes dl from Z (one more read of Z, which the frozen path never pays), so the
// head_bwd_kernel instances stay as they are.  One wave per pixel as above, 64 pixels a workgroup (16 a wave, loaded
// four -- two at 1024 channels -- at a time); a lane keeps sum_p dl[p][k] zn_p[c] for its NV channels of KB bins:
// KB x NV = 128 accumulators at both widths (KB = 16 at 512 channels: one pass; KB = 8 at 1024: two passes over the
// wave's pixels, the second with dl and 1 / ||z|| from LDS).  The four waves' sums meet in LDS in wave order, the
// workgroup stores part[block] = [NB][CH] sums then 16 dot slots (plain stores), and head_text_finalize_kernel adds the
// blocks in head_bias_finalize_kernel's fixed order: bit-reproducible, no float atomics.
constexpr int HEAD_TXT_PPB = 64;

template <int CH>
constexpr int head_txt_kb() { return CH <= 512 ? 16 : 8; }

// floats of one workgroup's partial: [NB][CH] sums, then the bins' dot slots padded to 16 (rows stay float4-aligned);
// 32 slots in the wide kernel's partials
__host__ __device__ inline size_t head_txt_stride(int NB, int CH, int pad = 16) { return (size_t)NB * CH + pad; }

template <class TZ, int CH>
__global__ __launch_bounds__(256) void head_text_bwd_kernel(const TZ* __restrict__ Z, const float* text, const float* logit_scale,
                                                            const float* anchors, const float* dlogits, const float* dexp,
                                                            const float* gscale, float* __restrict__ part, int P, int HW, int NB)
{
    constexpr int NV = CH / 64, KB = head_txt_kb<CH>(), PPW = HEAD_TXT_PPB / 4, G = 32 / NV;
    extern __shared__ __attribute__((aligned(16))) float tn[];
    float* red = tn + NB * CH;              // [KB][CH]: the waves' sums, combined in wave order
    float* dl_l = red + KB * CH;            // [4 waves][PPW][16]
    float* inv_l = dl_l + 4 * PPW * 16;     // [4][PPW]
    float* dot_l = inv_l + 4 * PPW;         // [4][16]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float s = expf(*logit_scale);
    const float gs = gscale ? *gscale : 1.0f;
    load_text<CH>(text, NB, tn);
    float* pblk = part + (size_t)blockIdx.x * head_txt_stride(NB, CH);
    float dots[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) dots[k] = 0.f;
    for (int k0 = 0; k0 < NB; k0 += KB) {
        float acc[KB][NV];
#pragma unroll
        for (int kk = 0; kk < KB; ++kk)
#pragma unroll
            for (int j = 0; j < NV; ++j) acc[kk][j] = 0.f;
        for (int i0 = 0; i0 < PPW; i0 += G) {
            const int p0 = blockIdx.x * HEAD_TXT_PPB + w + 4 * i0;
            if (p0 >= P) break;
            float vv[G][NV];
#pragma unroll
            for (int g = 0; g < G; ++g) load_pix<TZ, CH>(Z + (size_t)min(p0 + 4 * g, P - 1) * CH, vv[g]);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int p = p0 + 4 * g, i = i0 + g;
                if (p >= P) continue;
                float* v = vv[g];
                float dlr[KB], inv;
                if (KB >= 16 || k0 == 0) {
                    float ss = 0.f;
#pragma unroll
                    for (int j = 0; j < NV; ++j) ss += v[j] * v[j];
                    inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
                    float zs[NV];
#pragma unroll
                    for (int j = 0; j < NV; ++j) zs[j] = s * (v[j] * inv);
                    float lg[16], pr[16];
                    float mx = -INFINITY;
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        lg[k] = k < NB ? wave_sum(text_dot<CH>(tn + k * CH, zs)) : -INFINITY;
                        mx = fmaxf(mx, lg[k]);
                    }
                    float se = 0.f;
#pragma unroll
                    for (int k = 0; k < 16; ++k) { pr[k] = k < NB ? expf(lg[k] - mx) : 0.f; if (k < NB) se += pr[k]; }
                    float e = 0.f;
#pragma unroll
                    for (int k = 0; k < 16; ++k) if (k < NB) { pr[k] /= se; e += pr[k] * anchors[k]; }
                    const int b = p / HW, hw = p % HW;
                    const float de = dexp[(size_t)b * HW + hw] * gs;
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        if (k >= NB) continue;
                        // d logit_k, as in head_bwd_kernel
                        const float dl = dlogits[((size_t)b * NB + k) * HW + hw] * gs + de * pr[k] * (anchors[k] - e);
                        dots[k] += dl * lg[k];
                        if (k < KB) dlr[k % KB] = dl;
                        if (KB < 16 && lane == 0) dl_l[(w * PPW + i) * 16 + k] = dl;
                    }
                    if (KB < 16 && lane == 0) inv_l[w * PPW + i] = inv;
                } else {
                    inv = inv_l[w * PPW + i];
#pragma unroll
                    for (int kk = 0; kk < KB; ++kk) dlr[kk] = k0 + kk < NB ? dl_l[(w * PPW + i) * 16 + k0 + kk] : 0.f;
                }
                float zn[NV];
#pragma unroll
                for (int j = 0; j < NV; ++j) zn[j] = v[j] * inv;
#pragma unroll
                for (int kk = 0; kk < KB; ++kk) {
                    if (k0 + kk >= NB) continue;
#pragma unroll
                    for (int j = 0; j < NV; ++j) acc[kk][j] += dlr[kk] * zn[j];
                }
            }
        }
        // ((wave 0 + wave 1) + wave 2) + wave 3, the last one straight to the block's partial rows
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) {
            if (w == ww) {
#pragma unroll
                for (int kk = 0; kk < KB; ++kk) {
                    if (k0 + kk >= NB) continue;
#pragma unroll
                    for (int q = 0; q < NV / 4; ++q) {
                        float4 a = make_float4(acc[kk][4 * q], acc[kk][4 * q + 1], acc[kk][4 * q + 2], acc[kk][4 * q + 3]);
                        float4* r = reinterpret_cast<float4*>(red + kk * CH + 256 * q + 4 * lane);
                        if (ww > 0) { const float4 o = *r; a.x = o.x + a.x; a.y = o.y + a.y; a.z = o.z + a.z; a.w = o.w + a.w; }
                        if (ww < 3) *r = a;
                        else *reinterpret_cast<float4*>(pblk + (size_t)(k0 + kk) * CH + 256 * q + 4 * lane) = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    // lane 0's dots are the wave's per-pixel sums (wave_sum results are lane-uniform)
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) dot_l[w * 16 + k] = dots[k];
    }
    __syncthreads();
    if (threadIdx.x < 16)
        pblk[(size_t)NB * CH + threadIdx.x] = threadIdx.x < NB ? (dot_l[threadIdx.x] + dot_l[16 + threadIdx.x]) +
                                                                  (dot_l[32 + threadIdx.x] + dot_l[48 + threadIdx.x]) : 0.f;
}

// dtext[k][c] from the blocks' partials: workgroup (x, k) sums columns 64 x .. 64 x + 63 of bin k and the bin's dot slot
// over the blocks exactly as head_bias_finalize_kernel does (8 waves x 8 interleaved chains, combined in a fixed order),
// then wave 0 applies exp(ls) and the F.normalize backward of text row k
template <int CH, int PAD = 16>
__global__ __launch_bounds__(512) void head_text_finalize_kernel(const float* __restrict__ part, int nblk, int NB,
                                                                 const float* __restrict__ text, const float* logit_scale,
                                                                 float* __restrict__ dtext)
{
    __shared__ float ws[8][64];
    __shared__ float wd[8];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = blockIdx.y, c = blockIdx.x * 64 + lane;
    const size_t stride = head_txt_stride(NB, CH, PAD);
    const float* pc = part + (size_t)k * CH + c;
    const float* pd = part + (size_t)NB * CH + k;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, d[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int b = w;
    for (; b + 56 < nblk; b += 64) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { s[j] += pc[(size_t)(b + 8 * j) * stride]; d[j] += pd[(size_t)(b + 8 * j) * stride]; }
    }
    for (int j = 0; b < nblk; b += 8, ++j) { s[j & 7] += pc[(size_t)b * stride]; d[j & 7] += pd[(size_t)b * stride]; }
    ws[w][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    if (lane == 0) wd[w] = ((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]));
    __syncthreads();
    if (w == 0) {
        float t = 0.f, dot = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { t += ws[j][lane]; dot += wd[j]; }
        const float* tk = text + (size_t)k * CH;
        float ss = 0.f;                                       // ||t_k||^2 in load_text's order
#pragma unroll
        for (int q = 0; q < CH / 256; ++q) {
            const float4 x = *reinterpret_cast<const float4*>(tk + 256 * q + 4 * lane);
            ss += (x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w);
        }
        const float nrm = sqrtf(wave_sum(ss));
        const float inv = 1.0f / fmaxf(nrm, 1e-12f);
        const float dtn = expf(*logit_scale) * t;
        dtext[(size_t)k * CH + c] = (nrm > 1e-12f ? dtn - (tk[c] * inv) * dot : dtn) * inv;
    }
}

// ---- d text for up to 32 bins (ebc_head_bwd_text_wide).  With 32 rows the layout above needs 32 x 1024 x 4 = 128 KiB
// of text rows plus 32 KiB of wave sums plus the dl slots: over a CU's 160 KiB.  So the normalised rows pass through a
// 64 KiB LDS window in groups of RG = 16384 / CH rows (32 at 512 channels: one group; 16 at 1024: two), and the work
// splits into three phases over the workgroup's 64 pixels (Z is re-read from L2 in each, 2 - 4 KB a pixel):
//   1. per group: every wave's pixels x the group's rows -> logits into lg_l (LDS), 1 / ||z|| into inv_l
//   2. per pixel: all NB logits from lg_l into registers, softmax / expectation / dl as head_bwd_kernel forms them;
//      dl overwrites the logits in lg_l, dl x logit accumulates into the bins' dot sums
//   3. per KB bins: sum_p dl[p][k] zn_p in KB x NV accumulators a lane, the four waves combined in wave order, exactly
//      as head_text_bwd_kernel's later passes
// Partials: [NB][CH] sums then 32 dot slots a workgroup; head_text_finalize_kernel<CH, 32> sums them in its fixed order.
// LDS: (min(NB, RG) + KB) x CH x 4 + 8.75 KiB: at most 104.75 KiB at either width, one workgroup a CU.
template <int CH>
constexpr int head_txtw_rows() { return 16384 / CH; }

template <class TZ, int CH>
__global__ __launch_bounds__(256) void head_text_wide_bwd_kernel(const TZ* __restrict__ Z, const float* text,
                                                                 const float* logit_scale, const float* anchors,
                                                                 const float* dlogits, const float* dexp, const float* gscale,
                                                                 float* __restrict__ part, int P, int HW, int NB)
{
    constexpr int NV = CH / 64, KB = head_txt_kb<CH>(), PPW = HEAD_TXT_PPB / 4, G = 32 / NV, RG = head_txtw_rows<CH>();
    constexpr int CAP = EBC_HEAD_MAX_BINS;
    extern __shared__ __attribute__((aligned(16))) float tn[];   // [min(NB, RG)][CH]: one group of normalised rows
    float* red = tn + min(NB, RG) * CH;     // [KB][CH]: the waves' sums, combined in wave order
    float* lg_l = red + KB * CH;            // [4 waves][PPW][CAP]: logits (phase 1), then dl
    float* inv_l = lg_l + 4 * PPW * CAP;    // [4][PPW]
    float* dot_l = inv_l + 4 * PPW;         // [4][CAP]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float s = expf(*logit_scale);
    const float gs = gscale ? *gscale : 1.0f;
    float* pblk = part + (size_t)blockIdx.x * head_txt_stride(NB, CH, CAP);
    // phase 1: logits
    for (int r0 = 0; r0 < NB; r0 += RG) {
        const int nr = min(RG, NB - r0);
        if (r0) __syncthreads();            // every wave is done with the previous group
        load_text<CH>(text + (size_t)r0 * CH, nr, tn);
        for (int i0 = 0; i0 < PPW; i0 += G) {
            const int p0 = blockIdx.x * HEAD_TXT_PPB + w + 4 * i0;
            if (p0 >= P) break;
            float vv[G][NV];
#pragma unroll
            for (int g = 0; g < G; ++g) load_pix<TZ, CH>(Z + (size_t)min(p0 + 4 * g, P - 1) * CH, vv[g]);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int p = p0 + 4 * g, i = i0 + g;
                if (p >= P) continue;
                float* v = vv[g];
                float ss = 0.f;
#pragma unroll
                for (int j = 0; j < NV; ++j) ss += v[j] * v[j];
                const float inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
                float zs[NV];
#pragma unroll
                for (int j = 0; j < NV; ++j) zs[j] = s * (v[j] * inv);
                for (int kk = 0; kk < nr; ++kk) {
                    const float l = wave_sum(text_dot<CH>(tn + kk * CH, zs));
                    if (lane == 0) lg_l[(w * PPW + i) * CAP + r0 + kk] = l;
                }
                if (r0 == 0 && lane == 0) inv_l[w * PPW + i] = inv;
            }
        }
    }
    __syncthreads();
    // phase 2: dl of the wave's own pixels (every lane computes the same values, as in head_text_bwd_kernel)
    float dots[CAP];
#pragma unroll
    for (int k = 0; k < CAP; ++k) dots[k] = 0.f;
    for (int i = 0; i < PPW; ++i) {
        const int p = blockIdx.x * HEAD_TXT_PPB + w + 4 * i;
        if (p >= P) break;
        float* row = lg_l + (w * PPW + i) * CAP;
        float lg[CAP], pr[CAP];
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < CAP; ++k) {
            lg[k] = k < NB ? row[k] : -INFINITY;
            mx = fmaxf(mx, lg[k]);
        }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < CAP; ++k) { pr[k] = k < NB ? expf(lg[k] - mx) : 0.f; if (k < NB) se += pr[k]; }
        float e = 0.f;
#pragma unroll
        for (int k = 0; k < CAP; ++k) if (k < NB) { pr[k] /= se; e += pr[k] * anchors[k]; }
        const int b = p / HW, hw = p % HW;
        const float de = dexp[(size_t)b * HW + hw] * gs;
#pragma unroll
        for (int k = 0; k < CAP; ++k) {
            if (k >= NB) continue;
            // d logit_k, as in head_bwd_kernel
            const float dl = dlogits[((size_t)b * NB + k) * HW + hw] * gs + de * pr[k] * (anchors[k] - e);
            dots[k] += dl * lg[k];
            if (lane == 0) row[k] = dl;
        }
    }
    __syncthreads();
    // phase 3: sum_p dl[p][k] zn_p, KB bins a pass
    for (int k0 = 0; k0 < NB; k0 += KB) {
        float acc[KB][NV];
#pragma unroll
        for (int kk = 0; kk < KB; ++kk)
#pragma unroll
            for (int j = 0; j < NV; ++j) acc[kk][j] = 0.f;
        for (int i0 = 0; i0 < PPW; i0 += G) {
            const int p0 = blockIdx.x * HEAD_TXT_PPB + w + 4 * i0;
            if (p0 >= P) break;
            float vv[G][NV];
#pragma unroll
            for (int g = 0; g < G; ++g) load_pix<TZ, CH>(Z + (size_t)min(p0 + 4 * g, P - 1) * CH, vv[g]);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int p = p0 + 4 * g, i = i0 + g;
                if (p >= P) continue;
                const float inv = inv_l[w * PPW + i];
                float dlr[KB];
#pragma unroll
                for (int kk = 0; kk < KB; ++kk) dlr[kk] = k0 + kk < NB ? lg_l[(w * PPW + i) * CAP + k0 + kk] : 0.f;
                float zn[NV];
#pragma unroll
                for (int j = 0; j < NV; ++j) zn[j] = vv[g][j] * inv;
#pragma unroll
                for (int kk = 0; kk < KB; ++kk) {
                    if (k0 + kk >= NB) continue;
#pragma unroll
                    for (int j = 0; j < NV; ++j) acc[kk][j] += dlr[kk] * zn[j];
                }
            }
        }
        // ((wave 0 + wave 1) + wave 2) + wave 3, the last one straight to the block's partial rows
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) {
            if (w == ww) {
#pragma unroll
                for (int kk = 0; kk < KB; ++kk) {
                    if (k0 + kk >= NB) continue;
#pragma unroll
                    for (int q = 0; q < NV / 4; ++q) {
                        float4 a = make_float4(acc[kk][4 * q], acc[kk][4 * q + 1], acc[kk][4 * q + 2], acc[kk][4 * q + 3]);
                        float4* r = reinterpret_cast<float4*>(red + kk * CH + 256 * q + 4 * lane);
                        if (ww > 0) { const float4 o = *r; a.x = o.x + a.x; a.y = o.y + a.y; a.z = o.z + a.z; a.w = o.w + a.w; }
                        if (ww < 3) *r = a;
                        else *reinterpret_cast<float4*>(pblk + (size_t)(k0 + kk) * CH + 256 * q + 4 * lane) = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    // lane 0's dots are the wave's per-pixel sums (wave_sum results are lane-uniform)
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < CAP; ++k) dot_l[w * CAP + k] = dots[k];
    }
    __syncthreads();
    if (threadIdx.x < CAP)
        pblk[(size_t)NB * CH + threadIdx.x] = threadIdx.x < NB ? (dot_l[threadIdx.x] + dot_l[CAP + threadIdx.x]) +
                                                                  (dot_l[2 * CAP + threadIdx.x] + dot_l[3 * CAP + threadIdx.x]) : 0.f;
}

// ------------------------------------------------------------------------------- launchers
// Dynamic LDS in bytes of each kernel at NB bins: the launch's size and, at the instance's most bins, what ensure_lds
// opts the kernel in for.
template <int CH>
constexpr size_t head_fwd_lds(int NB) { return (size_t)NB * CH * 4; }                       // the text rows
template <int CH>
constexpr size_t head_bwd_lds(int NB) { return ((size_t)NB * CH + 4 * CH + 4) * 4; }        // + dbias_l, dsc_l
// the text rows (WIDE: one group of them), red, the dl / logit slots, inv_l, dot_l: at most 69 KiB / 101 KiB at 512 /
// 1024 channels, WIDE 104.75 KiB at either width
template <int CH, bool WIDE>
constexpr size_t head_txt_lds(int NB)
{
    constexpr int KB = head_txt_kb<CH>(), PPW = HEAD_TXT_PPB / 4, SLOTS = WIDE ? EBC_HEAD_MAX_BINS : 16;
    const int rows = WIDE && NB > head_txtw_rows<CH>() ? head_txtw_rows<CH>() : NB;
    return ((size_t)rows * CH + KB * CH + 4 * PPW * SLOTS + 4 * PPW + 4 * SLOTS) * 4;
}

// launch(CAP) with the capacity of the per-pixel register arrays as a constant: 16 up to 16 bins (the instance such a
// call always ran), EBC_HEAD_MAX_BINS above
template <class F>
int head_with_cap(int NB, F&& launch)
{
    if (NB > 16) return launch(std::integral_constant<int, EBC_HEAD_MAX_BINS>{});
    return launch(std::integral_constant<int, 16>{});
}

template <int CH>
int head_fwd_launch(int dtype_z, const void* Z, const float* text, const float* logit_scale, const float* anchors,
                    float* logits, float* expo, int P, int HW, int NB, hipStream_t st)
{
    const dim3 grid((P + HEAD_FWD_PPB - 1) / HEAD_FWD_PPB);
    return head_with_cap(NB, [&](auto cap) -> int {
        constexpr int CAP = decltype(cap)::value;
        // 17 .. 32 bins: up to 64 KiB (CH 512) / 128 KiB (CH 1024) of text rows; 16 bins never pass 64 KiB: no opt-in
        EBC_DTYPE_SWITCH(dtype_z,
            if constexpr (CAP > 16) {
                if (!ensure_lds<head_fwd_kernel<T, CH, CAP>>((int)head_fwd_lds<CH>(CAP), st)) return EBC_E_LAUNCH;
            }
            hipLaunchKernelGGL((head_fwd_kernel<T, CH, CAP>), grid, dim3(256), head_fwd_lds<CH>(NB), st, (const T*)Z, text,
                               logit_scale, anchors, logits, expo, P, HW, NB));
        EBC_CHECK_LAUNCH();
        return EBC_OK;
    });
}

// part: the blocks' d bias / d logit_scale partials (null: neither is wanted, no second launch)
template <int CH>
int head_bwd_launch(int dtype_z, int dtype_dz, const void* Z, const float* text, const float* logit_scale,
                    const float* anchors, const float* dlogits, const float* dexp, const float* gscale, void* dZ,
                    float* dbias, float* dscale, float* part, int P, int HW, int NB, hipStream_t st)
{
    const int nblk = (P + HEAD_BWD_PPB - 1) / HEAD_BWD_PPB;
    EBC_TRY(head_with_cap(NB, [&](auto cap) -> int {
        constexpr int CAP = decltype(cap)::value;
        // embed 1024: 81 KiB at 16 bins, up to 144 KiB at 32 (one workgroup a CU).  The dZ element type is the caller's
        // buffer type (dtype_dz), independent of Z's
        EBC_DTYPE_SWITCH(dtype_z, using TZ = T; EBC_DTYPE_SWITCH(dtype_dz,
            if (!ensure_lds<head_bwd_kernel<TZ, T, CH, CAP>>((int)head_bwd_lds<CH>(CAP), st)) return EBC_E_LAUNCH;
            hipLaunchKernelGGL((head_bwd_kernel<TZ, T, CH, CAP>), dim3(nblk), dim3(256), head_bwd_lds<CH>(NB), st,
                               (const TZ*)Z, text, logit_scale, anchors, dlogits, dexp, gscale, (T*)dZ, part, P, HW, NB)));
        EBC_CHECK_LAUNCH();
        return EBC_OK;
    }));
    if (part) {
        hipLaunchKernelGGL(head_bias_finalize_kernel<CH>, dim3(CH / 64 + 1), dim3(512), 0, st, part, nblk, dbias, dscale);
        EBC_CHECK_LAUNCH();
    }
    return EBC_OK;
}

// bytes of the text gradient's partials, `slots` dot slots a workgroup (also the most bins of that entry point)
size_t head_txt_ws_bytes(int P, int NB, int embed, int slots)
{
    if (P <= 0 || NB <= 0 || NB > slots || (embed != 512 && embed != 1024)) return 0;
    return (size_t)((P + HEAD_TXT_PPB - 1) / HEAD_TXT_PPB) * head_txt_stride(NB, embed, slots) * sizeof(float);
}

// d text: the partial kernel (WIDE: head_text_wide_bwd_kernel, 32 dot slots a partial; else head_text_bwd_kernel, 16),
// then the fixed-order sum over the blocks; one probe record over both
template <int CH, bool WIDE>
int head_bwd_text_launch(int dtype_z, const void* Z, const float* text, const float* logit_scale, const float* anchors,
                         const float* dlogits, const float* dexp, const float* gscale, float* dtext, int P, int HW, int NB,
                         void* ws, hipStream_t st)
{
    constexpr int SLOTS = WIDE ? EBC_HEAD_MAX_BINS : 16;
    const int nblk = (P + HEAD_TXT_PPB - 1) / HEAD_TXT_PPB;
    float* part = reinterpret_cast<float*>(ws);
    const size_t lds = head_txt_lds<CH, WIDE>(NB);
    constexpr int LDS_MAX = (int)head_txt_lds<CH, WIDE>(SLOTS);
    const ProbeScope probe(EBC_PROBE_HEAD_BWD_TEXT, 0, 0, 0, 0, P, NB, CH, st);
    EBC_DTYPE_SWITCH(dtype_z,
        constexpr auto kernel = WIDE ? head_text_wide_bwd_kernel<T, CH> : head_text_bwd_kernel<T, CH>;
        if (!ensure_lds<kernel>(LDS_MAX, st)) return EBC_E_LAUNCH;
        hipLaunchKernelGGL(kernel, dim3(nblk), dim3(256), lds, st, (const T*)Z, text, logit_scale, anchors, dlogits, dexp,
                           gscale, part, P, HW, NB));
    EBC_CHECK_LAUNCH();
    hipLaunchKernelGGL((head_text_finalize_kernel<CH, SLOTS>), dim3(CH / 64, NB), dim3(512), 0, st, part, nblk, NB, text,
                       logit_scale, dtext);
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

}  // namespace

// ---------------------------------------------------------------------------- entry points
// Each validates on the host, before any device work, then launches.
extern "C" int ebc_head_fwd(int dtype_z, const void* Z, const float* text, const float* logit_scale, const float* anchors,
                            float* logits, float* expo, int P, int HW, int NB, int embed, ebc_stream_t stream)
{
    if (!Z || !text || !logit_scale || !anchors || !logits || !expo) return EBC_E_ARG;
    if (P <= 0 || HW <= 0 || P % HW) return EBC_E_ARG;
    if (NB <= 0 || NB > EBC_HEAD_MAX_BINS || (embed != 512 && embed != 1024)) return EBC_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (embed == 512) return head_fwd_launch<512>(dtype_z, Z, text, logit_scale, anchors, logits, expo, P, HW, NB, st);
    return head_fwd_launch<1024>(dtype_z, Z, text, logit_scale, anchors, logits, expo, P, HW, NB, st);
}

// d bias / d logit_scale as per-block partials summed in block order by a second launch
extern "C" size_t ebc_head_bwd_workspace_bytes(int P, int embed)
{
    return P > 0 ? (size_t)((P + HEAD_BWD_PPB - 1) / HEAD_BWD_PPB) * (embed + 1) * sizeof(float) : 0;
}

extern "C" int ebc_head_bwd(int dtype_z, int dtype_dz, const void* Z, const float* text, const float* logit_scale,
                            const float* anchors, const float* dlogits, const float* dexp, const float* gscale, void* dZ,
                            float* dbias, float* dscale, int P, int HW, int NB, int embed, void* workspace,
                            size_t workspace_bytes, ebc_stream_t stream)
{
    if (!Z || !text || !logit_scale || !anchors || !dlogits || !dexp || !dZ) return EBC_E_ARG;
    if (P <= 0 || HW <= 0 || P % HW) return EBC_E_ARG;
    if (NB <= 0 || NB > EBC_HEAD_MAX_BINS || (embed != 512 && embed != 1024)) return EBC_E_UNSUPPORTED;
    const bool sums = dbias || dscale;
    if (sums && (!workspace || workspace_bytes < ebc_head_bwd_workspace_bytes(P, embed))) return EBC_E_ARG;
    float* part = sums ? reinterpret_cast<float*>(workspace) : nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (embed == 512)
        return head_bwd_launch<512>(dtype_z, dtype_dz, Z, text, logit_scale, anchors, dlogits, dexp, gscale, dZ, dbias,
                                    dscale, part, P, HW, NB, st);
    return head_bwd_launch<1024>(dtype_z, dtype_dz, Z, text, logit_scale, anchors, dlogits, dexp, gscale, dZ, dbias, dscale,
                                 part, P, HW, NB, st);
}

extern "C" size_t ebc_head_bwd_text_workspace_bytes(int P, int NB, int embed)
{
    return head_txt_ws_bytes(P, NB, embed, 16);
}

extern "C" int ebc_head_bwd_text(int dtype_z, const void* Z, const float* text, const float* logit_scale,
                                 const float* anchors, const float* dlogits, const float* dexp, const float* gscale,
                                 float* dtext, int P, int HW, int NB, int embed, void* workspace, size_t workspace_bytes,
                                 ebc_stream_t stream)
{
    if (!Z || !text || !logit_scale || !anchors || !dlogits || !dexp || !dtext) return EBC_E_ARG;
    if (P <= 0 || HW <= 0 || P % HW) return EBC_E_ARG;
    if (NB <= 0 || NB > 16 || (embed != 512 && embed != 1024)) return EBC_E_UNSUPPORTED;
    if (dtype_z != EBC_F32 && dtype_z != EBC_F16 && dtype_z != EBC_BF16) return EBC_E_ARG;
    if (!workspace || workspace_bytes < head_txt_ws_bytes(P, NB, embed, 16)) return EBC_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (embed == 512)
        return head_bwd_text_launch<512, false>(dtype_z, Z, text, logit_scale, anchors, dlogits, dexp, gscale, dtext, P, HW,
                                                NB, workspace, st);
    return head_bwd_text_launch<1024, false>(dtype_z, Z, text, logit_scale, anchors, dlogits, dexp, gscale, dtext, P, HW, NB,
                                             workspace, st);
}

extern "C" size_t ebc_head_bwd_text_wide_workspace_bytes(int P, int NB, int embed)
{
    return head_txt_ws_bytes(P, NB, embed, EBC_HEAD_MAX_BINS);
}

extern "C" int ebc_head_bwd_text_wide(int dtype_z, const void* Z, const float* text, const float* logit_scale,
                                      const float* anchors, const float* dlogits, const float* dexp, const float* gscale,
                                      float* dtext, int P, int HW, int NB, int embed, void* workspace,
                                      size_t workspace_bytes, ebc_stream_t stream)
{
    if (!Z || !text || !logit_scale || !anchors || !dlogits || !dexp || !dtext) return EBC_E_ARG;
    if (P <= 0 || HW <= 0 || P % HW) return EBC_E_ARG;
    if (NB <= 0 || NB > EBC_HEAD_MAX_BINS || (embed != 512 && embed != 1024)) return EBC_E_UNSUPPORTED;
    if (dtype_z != EBC_F32 && dtype_z != EBC_F16 && dtype_z != EBC_BF16) return EBC_E_ARG;
    if (!workspace || workspace_bytes < head_txt_ws_bytes(P, NB, embed, EBC_HEAD_MAX_BINS)) return EBC_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (embed == 512)
        return head_bwd_text_launch<512, true>(dtype_z, Z, text, logit_scale, anchors, dlogits, dexp, gscale, dtext, P, HW,
                                               NB, workspace, st);
    return head_bwd_text_launch<1024, true>(dtype_z, Z, text, logit_scale, anchors, dlogits, dexp, gscale, dtext, P, HW, NB,
                                            workspace, st);
}
