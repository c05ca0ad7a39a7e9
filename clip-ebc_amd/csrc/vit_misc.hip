// Memory-bound pieces of the CLIP-EBC ViT path on gfx950: LayerNorm fwd/bwd, patch im2col,
// token embedding (+CLS, +pos, ln_pre, VPT rows), VPT gradient, and the blockwise
// image-text similarity head fwd/bwd.
//
// Reference: LayerNorm (fp32 math)        models/clip/_clip/blocks.py:8-14
//            token prologue               models/clip/model.py:147-158, image_encoder.py:141-148
//            VPT assemble / disassemble   models/clip/model.py:131-140, 161-183
//            ln_post + drop CLS           models/clip/model.py:185-188
//            similarity head              models/clip/model.py:198-217
// Every kernel is one wave per row (D = 256*NV), 16-B vector accesses, fp32 statistics.
#include <climits>
#include "ebc_common.h"
#include "kernels.h"
#include "mfma.h"
#include "touch.h"
#include "vec_io.h"

using namespace ebc;

namespace {

constexpr float LN_EPS = 1e-5f;

struct RowMap {            // out row r -> source row (r / rpg) * gstride + goff + r % rpg
    int rpg, gstride, goff;
    __device__ __forceinline__ size_t operator()(int r) const {
        return (size_t)(r / rpg) * gstride + goff + (r % rpg);
    }
};

// Normalise NV float4 per lane of one row held in registers.
template <int NV>
__device__ __forceinline__ void ln_row(float4 (&v)[NV], const float4 (&gb)[2 * NV], float& mean, float& rstd) {
    constexpr float inv = 1.0f / (256.0f * NV);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    mean = wave_sum(s) * inv;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
        q += (a * a + b * b) + (c * c + d * d);
    }
    rstd = 1.0f / sqrtf(wave_sum(q) * inv + LN_EPS);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float4 g = gb[2 * i], b = gb[2 * i + 1];
        v[i] = make_float4((v[i].x - mean) * rstd * g.x + b.x, (v[i].y - mean) * rstd * g.y + b.y,
                           (v[i].z - mean) * rstd * g.z + b.z, (v[i].w - mean) * rstd * g.w + b.w);
    }
}

// Row blocks in XCD order (xcd_remap): each XCD takes a contiguous run of rows, the same rows the GEMM tiles that
// produce and consume them run on that XCD (gemm.hip maps its tiles the same way), so the row operands a kernel
// reads were last written on its own XCD
__device__ __forceinline__ int row_block() { return xcd_remap(blockIdx.x, (int)gridDim.x); }

// deep-VPT insert fused into ln_1 (model.py:131-140, 161-168): rows 1..NV of every crop are read from
// the prompt (vpt + b * bstride + (l-1) * D) instead of X, and written into X for the residual path
struct VptIns {
    const float* vpt;       // null: plain LayerNorm
    long bstride;
    int L, NV;
    float* X;
};

template <class T, int NV>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, RowMap map, const float* gamma,
                                                     const float* beta, T* out, float* outf, float* mean_out,
                                                     float* rstd_out, int M, VptIns vi)
{
    constexpr int D = 256 * NV;
    const int r = row_block() * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const float* xr = x + map(r) * D;
    bool ins = false;
    if (vi.vpt) {
        const int b = r / vi.L, l = r - b * vi.L;
        if (l >= 1 && l <= vi.NV) { xr = vi.vpt + b * vi.bstride + (size_t)(l - 1) * D; ins = true; }
    }
    float4 v[NV], gb[2 * NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = *reinterpret_cast<const float4*>(xr + 4 * lane + 256 * i);
    // gamma / beta issued with the row (not after the two reductions): one dependent L2 round trip fewer
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        gb[2 * i] = *reinterpret_cast<const float4*>(gamma + 4 * lane + 256 * i);
        gb[2 * i + 1] = *reinterpret_cast<const float4*>(beta + 4 * lane + 256 * i);
    }
    if (ins) {
#pragma unroll
        for (int i = 0; i < NV; ++i) *reinterpret_cast<float4*>(vi.X + (size_t)r * D + 4 * lane + 256 * i) = v[i];
    }
    float mean, rstd;
    ln_row<NV>(v, gb, mean, rstd);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const size_t o = (size_t)r * D + 4 * lane + 256 * i;
        if (out) st4<T>(out + o, v[i]);
        if (outf) st4<float>(outf + o, v[i]);
    }
    if (lane == 0 && mean_out) { mean_out[r] = mean; rstd_out[r] = rstd; }
}

// dx_out = dx_in + LN'(dy):  rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma
// deep-VPT gradient fused into ln_1's backward (model.py:131-140): rows 1..NV of every crop are the
// gradient of that layer's prompt tokens; they go to rows[(b*NV + l-1)*D] and the token-stream
// gradient of those rows (dx_out, dx_out_t) becomes zero (the prompt replaced them at this layer's input)
struct VptOut {
    float* rows;            // null: plain LayerNorm backward
    int L, NV;
};

// RD: rows-dense output (layer 0's prompt rows): x, dx_in, mean and rstd at the mapped row, dy and dx_out dense
// touch (ZF, ln_post's backward, the ViT backward's first launch): the first block's dX weights read onto the die
// (touch.h) -- the later blocks' are touched by the attention backward above them, the first block's had none (r06
// kernel trace: its c_fc dX product 38.3 us against 29 us for the others)
template <class T, class DY, int NV, bool ZF = false, bool RD = false>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const DY* __restrict__ dy, const float* __restrict__ x, RowMap map,
                                                     const float* mean_in, const float* rstd_in, const float* gamma,
                                                     const float* dx_in, float* dx_out, T* dx_out_t, int M, VptOut vo,
                                                     TouchList touch)
{
    constexpr int D = 256 * NV;
    constexpr float inv = 1.0f / (float)D;
    int r = row_block() * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    // the touch loads first: in flight beside the row's loads (issued after them, hipcc's waits for the row data at
    // the kernel-argument branches below drained them too), waited at the wave's end
    TouchSink ts;
    if constexpr (ZF) { if (touch.n) touch_issue1<4>(touch, ts); }
    if constexpr (ZF) {
        // grid over every destination row (M = groups * gstride): rows outside the mapped groups get a zero
        // gradient (ln_post: the CLS / prompt rows), the others run as mapped row r = their index in the groups
        if (r >= M) {
            if (touch.n) touch_wait(ts);
            return;
        }
        const int grp = r / map.gstride, l = r - grp * map.gstride;
        if (l < map.goff || l >= map.goff + map.rpg) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = 4 * lane + 256 * i;
                *reinterpret_cast<float4*>(dx_out + (size_t)r * D + c) = make_float4(0.f, 0.f, 0.f, 0.f);
                if (dx_out_t) st4<T>(dx_out_t + (size_t)r * D + c, make_float4(0.f, 0.f, 0.f, 0.f));
            }
            if (touch.n) touch_wait(ts);
            return;
        }
        r = grp * map.rpg + l - map.goff;
    } else {
        if (r >= M) return;
    }
    const size_t mrow = map(r), xr = mrow * D;
    const float mean = mean_in[RD ? mrow : r], rstd = rstd_in[RD ? mrow : r];
    const size_t orow = RD ? (size_t)r * D : xr;
    float4 g[NV], xh[NV], din[NV];
    float s1 = 0.f, s2 = 0.f;
    // the incoming gradient is loaded with the row operands (not after the reductions)
#pragma unroll
    for (int i = 0; i < NV; ++i)
        din[i] = dx_in ? *reinterpret_cast<const float4*>(dx_in + xr + 4 * lane + 256 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = 4 * lane + 256 * i;
        const float4 d = ld4<DY>(dy + (size_t)r * D + c);
        const float4 gm = *reinterpret_cast<const float4*>(gamma + c);
        const float4 xv = *reinterpret_cast<const float4*>(x + xr + c);
        g[i] = make_float4(d.x * gm.x, d.y * gm.y, d.z * gm.z, d.w * gm.w);
        xh[i] = make_float4((xv.x - mean) * rstd, (xv.y - mean) * rstd, (xv.z - mean) * rstd, (xv.w - mean) * rstd);
        s1 += (g[i].x + g[i].y) + (g[i].z + g[i].w);
        s2 += (g[i].x * xh[i].x + g[i].y * xh[i].y) + (g[i].z * xh[i].z + g[i].w * xh[i].w);
    }
    s1 = wave_sum(s1) * inv;
    s2 = wave_sum(s2) * inv;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = 4 * lane + 256 * i;
        float4 o = make_float4(rstd * (g[i].x - s1 - xh[i].x * s2), rstd * (g[i].y - s1 - xh[i].y * s2),
                               rstd * (g[i].z - s1 - xh[i].z * s2), rstd * (g[i].w - s1 - xh[i].w * s2));
        if (dx_in) { o.x += din[i].x; o.y += din[i].y; o.z += din[i].z; o.w += din[i].w; }
        if (vo.rows) {
            const int b = r / vo.L, l = r - b * vo.L;
            if (l >= 1 && l <= vo.NV) {
                *reinterpret_cast<float4*>(vo.rows + ((size_t)b * vo.NV + l - 1) * D + c) = o;
                o = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        *reinterpret_cast<float4*>(dx_out + orow + c) = o;
        if (!RD && dx_out_t) st4<T>(dx_out_t + xr + c, o);
    }
    if constexpr (ZF) { if (touch.n) touch_wait(ts); }
}

// dvpt_l[r][c] = sum_b rows_l[b][r][c] for every layer l with a destination (crop order), one launch
struct VptSum {
    float* dst[64];
};
__global__ void vpt_sum_kernel(const float* __restrict__ rows, VptSum vs, int layers, int B, int n4)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;        // float4 index within one layer's [NV][D]
    const int l = blockIdx.y;
    if (e >= n4 || !vs.dst[l]) return;
    const float4* src = reinterpret_cast<const float4*>(rows) + (size_t)l * B * n4 + e;
    // sixteen crops' loads in flight before their adds (r06: one dependent HBM round trip per crop took 10 us a step;
    // batches of eight left the 16-crop step's last seven crops one load at a time): indices past B re-read the last
    // crop and are not added, and the adds keep crop order, so the sums keep their bits
    constexpr int NB = 16;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b0 = 0; b0 < B; b0 += NB) {
        float4 v[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) v[i] = src[(size_t)min(b0 + i, B - 1) * n4];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int b = b0 + i;
            if (b == 0) acc = v[i];
            else if (b < B) { acc.x += v[i].x; acc.y += v[i].y; acc.z += v[i].z; acc.w += v[i].w; }
        }
    }
    reinterpret_cast<float4*>(vs.dst[l])[e] = acc;
}

// x [B,3,H,W] f32 -> patches [B*gh*gw, 3*P*P] (k = c*P*P + kh*P + kw, conv1 weight order).  One workgroup a patch
// row, one float4 of it a thread, 32-bit index math (r06: the grid-stride form's 64-bit divisions made it VALU-bound,
// 9.1 us a step for 14 MB)
template <class T>
__global__ __launch_bounds__(1024) void im2col_kernel(const float* __restrict__ x, T* __restrict__ out, int H, int W, int P)
{
    const int gh = H / P, gw = W / P, PP = P * P, KD = 3 * PP;
    const int row = blockIdx.x, k = 4 * threadIdx.x;
    if (k >= KD) return;
    const int px = row % gw, t = row / gw, py = t % gh, b = t / gh;
    const int c = k / PP, r = k - c * PP, kh = r / P, kw = r - kh * P;
    const float4 v = *reinterpret_cast<const float4*>(x + ((size_t)(b * 3 + c) * H + (py * P + kh)) * W + px * P + kw);
    st4<T>(out + (size_t)row * KD + k, v);
}

// X[b, s] for the first block (models/clip/model.py:147-168):
//   s = 0: ln_pre(cls + pos[0]);  1 <= s <= NVPT: vpt_0;  s > NVPT: ln_pre(patch[b, s-1-NVPT] + pos[s-NVPT])
template <int NV>
__global__ __launch_bounds__(256) void embed_kernel(const float* __restrict__ patch, const float* cls, const float* pos,
                                                    const float* gamma, const float* beta, const float* vpt,
                                                    long vpt_bstride, float* X, int B, int L, int G, int NVPT)
{
    constexpr int D = 256 * NV;
    const int r = row_block() * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= B * L) return;
    const int b = r / L, s = r % L;
    float* xo = X + (size_t)r * D;
    if (s >= 1 && s <= NVPT) {
        const float* vp = vpt + b * vpt_bstride + (size_t)(s - 1) * D;
#pragma unroll
        for (int i = 0; i < NV; ++i)
            *reinterpret_cast<float4*>(xo + 4 * lane + 256 * i) = *reinterpret_cast<const float4*>(vp + 4 * lane + 256 * i);
        return;
    }
    const int p = s == 0 ? -1 : s - 1 - NVPT;
    float4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = 4 * lane + 256 * i;
        const float4 e = p < 0 ? *reinterpret_cast<const float4*>(cls + c)
                               : *reinterpret_cast<const float4*>(patch + ((size_t)b * G + p) * D + c);
        const float4 q = *reinterpret_cast<const float4*>(pos + (size_t)(p + 1) * D + c);
        v[i] = make_float4(e.x + q.x, e.y + q.y, e.z + q.z, e.w + q.w);
    }
    float4 gb[2 * NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        gb[2 * i] = *reinterpret_cast<const float4*>(gamma + 4 * lane + 256 * i);
        gb[2 * i + 1] = *reinterpret_cast<const float4*>(beta + 4 * lane + 256 * i);
    }
    float mean, rstd;
    ln_row<NV>(v, gb, mean, rstd);
#pragma unroll
    for (int i = 0; i < NV; ++i) *reinterpret_cast<float4*>(xo + 4 * lane + 256 * i) = v[i];
}

// dvpt[r, c] (+)= sum_b dX[b, 1+r, c]  (or per batch when per_batch), then zero those rows of dX / dXt.
// Block = 64 column groups of 4 x 4 crop lanes for one 256-column chunk of prompt row r: crop lane bl sums
// crops bl, bl+4, ... (all its loads in flight at once), the 4 lane sums meet in LDS in lane order.
template <class T>
__global__ __launch_bounds__(256) void vpt_grad_kernel(float* __restrict__ dX, T* __restrict__ dXt,
                                                       float* __restrict__ dvpt, int B, int L, int NVPT, int D,
                                                       int per_batch, int accumulate)
{
    __shared__ float4 red[4][64];
    const int cg = threadIdx.x & 63, bl = threadIdx.x >> 6;
    const int chunks = D / 256, r = blockIdx.x / chunks, c = (blockIdx.x - r * chunks) * 256 + 4 * cg;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 s = z;
    constexpr int MAXB = 16;                      // crops per lane held in registers per pass
    for (int b0 = bl; b0 < B; b0 += 4 * MAXB) {
        float4 x[MAXB];
#pragma unroll
        for (int k = 0; k < MAXB; ++k) {
            const int b = b0 + 4 * k;
            x[k] = b < B ? *reinterpret_cast<const float4*>(dX + ((size_t)b * L + 1 + r) * D + c) : z;
        }
#pragma unroll
        for (int k = 0; k < MAXB; ++k) {
            const int b = b0 + 4 * k;
            if (b >= B) continue;
            const size_t o = ((size_t)b * L + 1 + r) * D + c;
            if (per_batch) {
                float4* dst = reinterpret_cast<float4*>(dvpt + ((size_t)b * NVPT + r) * D + c);
                float4 y = x[k];
                if (accumulate) { const float4 d = *dst; y.x += d.x; y.y += d.y; y.z += d.z; y.w += d.w; }
                *dst = y;
            } else {
                s.x += x[k].x; s.y += x[k].y; s.z += x[k].z; s.w += x[k].w;
            }
            *reinterpret_cast<float4*>(dX + o) = z;
            if (dXt) st4<T>(dXt + o, z);
        }
    }
    if (per_batch) return;
    red[bl][cg] = s;
    __syncthreads();
    if (bl == 0) {
        float4 t = red[0][cg];
#pragma unroll
        for (int k = 1; k < 4; ++k) { const float4 u = red[k][cg]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        float4* dst = reinterpret_cast<float4*>(dvpt + (size_t)r * D + c);
        if (accumulate) { const float4 d = *dst; t.x += d.x; t.y += d.y; t.z += d.z; t.w += d.w; }
        *dst = t;
    }
}

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
constexpr int HEAD_MAX_BINS = 32;

template <int CH>
constexpr int head_txtw_rows() { return 16384 / CH; }

template <class TZ, int CH>
__global__ __launch_bounds__(256) void head_text_wide_bwd_kernel(const TZ* __restrict__ Z, const float* text,
                                                                 const float* logit_scale, const float* anchors,
                                                                 const float* dlogits, const float* dexp, const float* gscale,
                                                                 float* __restrict__ part, int P, int HW, int NB)
{
    constexpr int NV = CH / 64, KB = head_txt_kb<CH>(), PPW = HEAD_TXT_PPB / 4, G = 32 / NV, RG = head_txtw_rows<CH>();
    constexpr int CAP = HEAD_MAX_BINS;
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

template <class T>
__global__ void cast_kernel(const float* in, T* out, size_t n4)
{
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n4; e += (size_t)gridDim.x * blockDim.x)
        st4<T>(out + 4 * e, reinterpret_cast<const float4*>(in)[e]);
}

inline int grid_for(size_t n, int block = 256) {
    const size_t g = (n + block - 1) / block;
    return (int)(g < 8192 ? (g ? g : 1) : 8192);
}

}  // namespace

// ------------------------------------------------------------------------------- launchers
namespace ebc {

// D = 768 (the ViT) or 512 (the text tower): NV = D / 256 float4 a lane
static int ln_fwd_launch(int dtype, const float* x, RowMap map, const float* gamma, const float* beta, void* out,
                         float* outf, float* mean, float* rstd, int M, VptIns vi, hipStream_t st, int D = 768)
{
    const dim3 grid((M + 3) / 4);
    const ProbeScope probe(EBC_PROBE_LN_FWD, 0, 0, 0, 0, M, D, 0, st);
    if (D == 512) {
        EBC_DTYPE_SWITCH(dtype, hipLaunchKernelGGL((ln_fwd_kernel<T, 2>), grid, dim3(256), 0, st, x, map, gamma, beta,
                                                   (T*)out, outf, mean, rstd, M, vi));
    } else {
        EBC_DTYPE_SWITCH(dtype, hipLaunchKernelGGL((ln_fwd_kernel<T, 3>), grid, dim3(256), 0, st, x, map, gamma, beta,
                                                   (T*)out, outf, mean, rstd, M, vi));
    }
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

int layernorm_fwd(int dtype, const float* x, int rpg, int gstride, int goff, const float* gamma, const float* beta,
                  void* out, float* outf, float* mean, float* rstd, int M, int D, hipStream_t st)
{
    if ((D != 768 && D != 512) || M <= 0) return EBC_E_UNSUPPORTED;
    const RowMap map{rpg > 0 ? rpg : M, gstride, goff};
    return ln_fwd_launch(dtype, x, map, gamma, beta, out, outf, mean, rstd, M, VptIns{nullptr, 0, 1, 0, nullptr}, st, D);
}

int layernorm_fwd_vpt(int dtype, float* X, const float* vpt, long vpt_bstride, int L, int NVPT, const float* gamma,
                      const float* beta, void* out, float* mean, float* rstd, int M, int D, hipStream_t st)
{
    if (D != 768 || M <= 0 || L <= NVPT || M % L) return EBC_E_UNSUPPORTED;
    const RowMap map{M, 0, 0};
    return ln_fwd_launch(dtype, X, map, gamma, beta, out, nullptr, mean, rstd, M,
                         VptIns{vpt, vpt_bstride, L, NVPT, X}, st);
}

template <class T, int NV = 3>
static int ln_bwd_t(int dy_f32, const void* dy, const float* x, RowMap map, const float* mean, const float* rstd,
                    const float* gamma, const float* dx_in, float* dx_out, void* dx_out_t, int M, VptOut vo, hipStream_t st)
{
    const dim3 grid((M + 3) / 4);
    const ProbeScope probe(EBC_PROBE_LN_BWD, 0, 0, 0, 0, M, 256 * NV, 0, st);
    if (dy_f32)
        hipLaunchKernelGGL((ln_bwd_kernel<T, float, NV>), grid, dim3(256), 0, st, (const float*)dy, x, map, mean, rstd, gamma, dx_in, dx_out, (T*)dx_out_t, M, vo, TouchList{});
    else
        hipLaunchKernelGGL((ln_bwd_kernel<T, T, NV>), grid, dim3(256), 0, st, (const T*)dy, x, map, mean, rstd, gamma, dx_in, dx_out, (T*)dx_out_t, M, vo, TouchList{});
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

// ln_post's backward (dy f32 over the patch rows, no incoming dx): also writes the zero gradient of every row
// outside the groups, so dx_out / dx_out_t need no memset: one launch over all M / rpg * gstride rows
int layernorm_bwd_fill(int dtype, const float* dy, const float* x, int rpg, int gstride, int goff, const float* mean,
                       const float* rstd, const float* gamma, float* dx_out, void* dx_out_t, int M, int D, hipStream_t st,
                       const TouchList* touch)
{
    if (D != 768 || M <= 0 || rpg <= 0 || M % rpg || goff + rpg > gstride) return EBC_E_UNSUPPORTED;
    const RowMap map{rpg, gstride, goff};
    const VptOut vo{nullptr, 1, 0};
    TouchList t = touch && touch_enabled() ? *touch : TouchList{};
    size_t lines = 0;                                   // at most one line a lane (touch_issue1)
    for (int i = 0; i < t.n; ++i) lines += t.bytes[i] >> 7;
    const int Mf = M / rpg * gstride;
    const dim3 grid((Mf + 3) / 4);
    if (lines > (size_t)grid.x * 256) t = TouchList{};
    {
        const ProbeScope probe(EBC_PROBE_LN_BWD, 0, 0, 0, 0, Mf, 768, 0, st);
        EBC_DTYPE_SWITCH(dtype, hipLaunchKernelGGL((ln_bwd_kernel<T, float, 3, true>), grid, dim3(256), 0, st, dy, x, map,
                                                   mean, rstd, gamma, nullptr, dx_out, (T*)dx_out_t, Mf, vo, t));
    }
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

int layernorm_bwd(int dtype, int dy_f32, const void* dy, const float* x, int rpg, int gstride, int goff,
                  const float* mean, const float* rstd, const float* gamma, const float* dx_in, float* dx_out,
                  void* dx_out_t, int M, int D, hipStream_t st)
{
    if ((D != 768 && D != 512) || M <= 0) return EBC_E_UNSUPPORTED;
    const RowMap map{rpg > 0 ? rpg : M, gstride, goff};
    const VptOut vo{nullptr, 1, 0};
    // f32: dy is always f32
    if (D == 512)
        EBC_DTYPE_SWITCH(dtype, return (ln_bwd_t<T, 2>(E::BYTES == 4 ? 1 : dy_f32, dy, x, map, mean, rstd, gamma, dx_in,
                                                       dx_out, dx_out_t, M, vo, st)));
    EBC_DTYPE_SWITCH(dtype, return ln_bwd_t<T>(E::BYTES == 4 ? 1 : dy_f32, dy, x, map, mean, rstd, gamma, dx_in, dx_out,
                                               dx_out_t, M, vo, st));
}

int im2col(int dtype, const float* x, void* out, int B, int H, int W, int P, hipStream_t st)
{
    if (H % P || W % P || (P * P * 3) % 4 || P % 4) return EBC_E_ARG;
    const long rows = (long)B * (H / P) * (W / P);
    const int k4 = 3 * P * P / 4, blk = (k4 + 63) / 64 * 64;
    if (rows <= 0 || rows > INT_MAX || blk > 1024 || (size_t)B * 3 * H * W > (size_t)INT_MAX * 4) return EBC_E_ARG;
    const dim3 grid((unsigned)rows);
    EBC_DTYPE_SWITCH(dtype, hipLaunchKernelGGL(im2col_kernel<T>, grid, dim3(blk), 0, st, x, (T*)out, H, W, P));
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

int embed_tokens(const float* patch, const float* cls, const float* pos, const float* gamma, const float* beta,
                 const float* vpt, long vpt_bstride, float* X, int B, int L, int G, int NVPT, int D, hipStream_t st)
{
    if (D != 768 || L != 1 + NVPT + G) return EBC_E_ARG;
    hipLaunchKernelGGL(embed_kernel<3>, dim3((B * L + 3) / 4), dim3(256), 0, st, patch, cls, pos, gamma, beta, vpt,
                       vpt_bstride, X, B, L, G, NVPT);
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

int layernorm_bwd_vpt(int dtype, const void* dy, const float* x, const float* mean, const float* rstd,
                      const float* gamma, const float* dx_in, float* dx_out, void* dx_out_t, int M, int D, float* vpt_rows,
                      int L, int NVPT, hipStream_t st)
{
    if (D != 768 || M <= 0 || M % L || NVPT < 1 || NVPT >= L || !vpt_rows) return EBC_E_UNSUPPORTED;
    const RowMap map{M, 0, 0};
    const VptOut vo{vpt_rows, L, NVPT};
    // dy in the compute dtype (f32: dy_f32 = 1)
    EBC_DTYPE_SWITCH(dtype, return ln_bwd_t<T>(E::BYTES == 4, dy, x, map, mean, rstd, gamma, dx_in, dx_out, dx_out_t, M, vo, st));
}

int layernorm_bwd_rows(int dtype, const void* dy, const float* x, int rpg, int gstride, int goff, const float* mean,
                       const float* rstd, const float* gamma, const float* dx_in, float* dx_out, int M, int D,
                       hipStream_t st)
{
    if (D != 768 || M <= 0 || rpg <= 0 || M % rpg || goff < 0 || goff + rpg > gstride) return EBC_E_UNSUPPORTED;
    const RowMap map{rpg, gstride, goff};
    const VptOut vo{nullptr, 1, 0};
    const dim3 grid((M + 3) / 4);
    const ProbeScope probe(EBC_PROBE_LN_BWD, 0, 0, 0, 0, M, 768, 0, st);
    EBC_DTYPE_SWITCH(dtype, hipLaunchKernelGGL((ln_bwd_kernel<T, T, 3, false, true>), grid, dim3(256), 0, st, (const T*)dy, x,
                                               map, mean, rstd, gamma, dx_in, dx_out, (T*)nullptr, M, vo, TouchList{}));
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

int vpt_sum(const float* rows, float* const* dst, int layers, int B, int NVPT, int D, hipStream_t st)
{
    if (layers <= 0 || layers > 64 || B <= 0 || D % 4) return EBC_E_ARG;
    VptSum vs{};
    bool any = false;
    for (int l = 0; l < layers; ++l) { vs.dst[l] = dst[l]; any |= dst[l] != nullptr; }
    if (!any) return EBC_OK;
    const int n4 = NVPT * D / 4;
    hipLaunchKernelGGL(vpt_sum_kernel, dim3((n4 + 255) / 256, layers), dim3(256), 0, st, rows, vs, layers, B, n4);
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

int vpt_grad(int dtype, float* dX, void* dXt, float* dvpt, int B, int L, int NVPT, int D, int per_batch, int accumulate, hipStream_t st)
{
    if (D % 256 || NVPT <= 0 || B <= 0) return NVPT == 0 ? EBC_OK : EBC_E_UNSUPPORTED;
    const dim3 grid((unsigned)(NVPT * (D / 256)));
    EBC_DTYPE_SWITCH(dtype, hipLaunchKernelGGL(vpt_grad_kernel<T>, grid, dim3(256), 0, st, dX, (T*)dXt, dvpt, B, L, NVPT, D,
                                               per_batch, accumulate));
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

template <int CH>
static int head_fwd_t(int dtype_z, const void* Z, const float* text, const float* logit_scale, const float* anchors,
                      float* logits, float* expo, int P, int HW, int NB, hipStream_t st)
{
    const dim3 grid((P + HEAD_FWD_PPB - 1) / HEAD_FWD_PPB);
    const size_t lds = (size_t)NB * CH * 4;
    if (NB > 16) {      // 17 .. 32 bins: the 32-slot instance; up to 64 KiB (CH 512) / 128 KiB (CH 1024) of text rows
        constexpr int LDS_MAX = HEAD_MAX_BINS * CH * 4;
        EBC_DTYPE_SWITCH(dtype_z,
            if (!ensure_lds<head_fwd_kernel<T, CH, HEAD_MAX_BINS>>(LDS_MAX, st)) return EBC_E_LAUNCH;
            hipLaunchKernelGGL((head_fwd_kernel<T, CH, HEAD_MAX_BINS>), grid, dim3(256), lds, st, (const T*)Z, text,
                               logit_scale, anchors, logits, expo, P, HW, NB));
        EBC_CHECK_LAUNCH();
        return EBC_OK;
    }
    EBC_DTYPE_SWITCH(dtype_z, hipLaunchKernelGGL((head_fwd_kernel<T, CH>), grid, dim3(256), lds, st, (const T*)Z, text,
                                                 logit_scale, anchors, logits, expo, P, HW, NB));
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

int head_fwd(int dtype_z, const void* Z, const float* text, const float* logit_scale, const float* anchors,
             float* logits, float* expo, int P, int HW, int NB, int embed, hipStream_t st)
{
    if (NB <= 0 || NB > HEAD_MAX_BINS) return EBC_E_UNSUPPORTED;
    if (embed == 512) return head_fwd_t<512>(dtype_z, Z, text, logit_scale, anchors, logits, expo, P, HW, NB, st);
    if (embed == 1024) return head_fwd_t<1024>(dtype_z, Z, text, logit_scale, anchors, logits, expo, P, HW, NB, st);
    return EBC_E_UNSUPPORTED;
}

template <int CH>
static int head_bwd_t(int dtype_z, int dtype_dz, const void* Z, const float* text, const float* logit_scale,
                      const float* anchors, const float* dlogits, const float* dexp, const float* gscale, void* dZ,
                      float* dbias, float* dscale, int P, int HW, int NB, void* ws, size_t wsb, hipStream_t st)
{
    const int nblk = (P + HEAD_BWD_PPB - 1) / HEAD_BWD_PPB;
    const bool sums = dbias || dscale;
    float* part = sums ? reinterpret_cast<float*>(ws) : nullptr;
    if (sums && (!ws || wsb < head_bwd_ws_bytes(P, CH))) return EBC_E_ARG;
    const dim3 grid(nblk);
    const size_t lds = ((size_t)NB * CH + 4 * CH + 4) * 4;
    constexpr int LDS_MAX = (16 * CH + 4 * CH + 4) * 4;      // NB <= 16 (embed 1024: 81 KiB)
    // the dZ element type is the caller's buffer type (dtype_dz), independent of Z's
    if (NB > 16) {      // 17 .. 32 bins: the 32-slot instance (embed 1024: up to 144 KiB, one workgroup a CU)
        constexpr int LDS_WIDE = (HEAD_MAX_BINS * CH + 4 * CH + 4) * 4;
        EBC_DTYPE_SWITCH(dtype_z, using TZ = T; EBC_DTYPE_SWITCH(dtype_dz,
            if (!ensure_lds<head_bwd_kernel<TZ, T, CH, HEAD_MAX_BINS>>(LDS_WIDE, st)) return EBC_E_LAUNCH;
            hipLaunchKernelGGL((head_bwd_kernel<TZ, T, CH, HEAD_MAX_BINS>), grid, dim3(256), lds, st, (const TZ*)Z, text,
                               logit_scale, anchors, dlogits, dexp, gscale, (T*)dZ, part, P, HW, NB)));
    } else {
        EBC_DTYPE_SWITCH(dtype_z, using TZ = T; EBC_DTYPE_SWITCH(dtype_dz,
            if (!ensure_lds<head_bwd_kernel<TZ, T, CH>>(LDS_MAX, st)) return EBC_E_LAUNCH;
            hipLaunchKernelGGL((head_bwd_kernel<TZ, T, CH>), grid, dim3(256), lds, st, (const TZ*)Z, text, logit_scale, anchors,
                               dlogits, dexp, gscale, (T*)dZ, part, P, HW, NB)));
    }
    EBC_CHECK_LAUNCH();
    if (sums) {
        hipLaunchKernelGGL(head_bias_finalize_kernel<CH>, dim3(CH / 64 + 1), dim3(512), 0, st, part, nblk, dbias, dscale);
        EBC_CHECK_LAUNCH();
    }
    return EBC_OK;
}

size_t head_bwd_ws_bytes(int P, int embed)
{
    return P > 0 ? (size_t)((P + HEAD_BWD_PPB - 1) / HEAD_BWD_PPB) * (embed + 1) * sizeof(float) : 0;
}

int head_bwd(int dtype_z, int dtype_dz, const void* Z, const float* text, const float* logit_scale, const float* anchors,
             const float* dlogits, const float* dexp, const float* gscale, void* dZ, float* dbias, float* dscale,
             int P, int HW, int NB, int embed, void* ws, size_t wsb, hipStream_t st)
{
    if (NB <= 0 || NB > HEAD_MAX_BINS || P <= 0) return EBC_E_UNSUPPORTED;
    if (embed == 512)
        return head_bwd_t<512>(dtype_z, dtype_dz, Z, text, logit_scale, anchors, dlogits, dexp, gscale, dZ, dbias, dscale, P, HW, NB,
                               ws, wsb, st);
    if (embed == 1024)
        return head_bwd_t<1024>(dtype_z, dtype_dz, Z, text, logit_scale, anchors, dlogits, dexp, gscale, dZ, dbias, dscale, P, HW,
                                NB, ws, wsb, st);
    return EBC_E_UNSUPPORTED;
}

size_t head_bwd_text_ws_bytes(int P, int NB, int embed)
{
    if (P <= 0 || NB <= 0 || embed <= 0) return 0;
    return (size_t)((P + HEAD_TXT_PPB - 1) / HEAD_TXT_PPB) * head_txt_stride(NB, embed) * sizeof(float);
}

template <int CH>
static int head_bwd_text_t(int dtype_z, const void* Z, const float* text, const float* logit_scale, const float* anchors,
                           const float* dlogits, const float* dexp, const float* gscale, float* dtext, int P, int HW,
                           int NB, void* ws, hipStream_t st)
{
    constexpr int KB = head_txt_kb<CH>(), PPW = HEAD_TXT_PPB / 4;
    const int nblk = (P + HEAD_TXT_PPB - 1) / HEAD_TXT_PPB;
    float* part = reinterpret_cast<float*>(ws);
    const size_t lds = ((size_t)NB * CH + KB * CH + 4 * PPW * 16 + 4 * PPW + 64) * 4;
    constexpr int LDS_MAX = (16 * CH + KB * CH + 4 * PPW * 16 + 4 * PPW + 64) * 4;    // 69 KiB / 101 KiB
    const ProbeScope probe(EBC_PROBE_HEAD_BWD_TEXT, 0, 0, 0, 0, P, NB, CH, st);
    EBC_DTYPE_SWITCH(dtype_z,
        if (!ensure_lds<head_text_bwd_kernel<T, CH>>(LDS_MAX, st)) return EBC_E_LAUNCH;
        hipLaunchKernelGGL((head_text_bwd_kernel<T, CH>), dim3(nblk), dim3(256), lds, st, (const T*)Z, text, logit_scale,
                           anchors, dlogits, dexp, gscale, part, P, HW, NB));
    EBC_CHECK_LAUNCH();
    hipLaunchKernelGGL(head_text_finalize_kernel<CH>, dim3(CH / 64, NB), dim3(512), 0, st, part, nblk, NB, text, logit_scale,
                       dtext);
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

int head_bwd_text(int dtype_z, const void* Z, const float* text, const float* logit_scale, const float* anchors,
                  const float* dlogits, const float* dexp, const float* gscale, float* dtext, int P, int HW, int NB,
                  int embed, void* ws, size_t wsb, hipStream_t st)
{
    if (NB <= 0 || NB > 16 || (embed != 512 && embed != 1024)) return EBC_E_UNSUPPORTED;
    if (dtype_z != EBC_F32 && dtype_z != EBC_F16 && dtype_z != EBC_BF16) return EBC_E_ARG;
    if (!ws || wsb < head_bwd_text_ws_bytes(P, NB, embed)) return EBC_E_ARG;
    if (embed == 512)
        return head_bwd_text_t<512>(dtype_z, Z, text, logit_scale, anchors, dlogits, dexp, gscale, dtext, P, HW, NB, ws, st);
    return head_bwd_text_t<1024>(dtype_z, Z, text, logit_scale, anchors, dlogits, dexp, gscale, dtext, P, HW, NB, ws, st);
}

size_t head_bwd_text_wide_ws_bytes(int P, int NB, int embed)
{
    if (P <= 0 || NB <= 0 || NB > HEAD_MAX_BINS || (embed != 512 && embed != 1024)) return 0;
    return (size_t)((P + HEAD_TXT_PPB - 1) / HEAD_TXT_PPB) * head_txt_stride(NB, embed, HEAD_MAX_BINS) * sizeof(float);
}

template <int CH>
static int head_bwd_text_wide_t(int dtype_z, const void* Z, const float* text, const float* logit_scale, const float* anchors,
                                const float* dlogits, const float* dexp, const float* gscale, float* dtext, int P, int HW,
                                int NB, void* ws, hipStream_t st)
{
    constexpr int KB = head_txt_kb<CH>(), PPW = HEAD_TXT_PPB / 4, RG = head_txtw_rows<CH>(), CAP = HEAD_MAX_BINS;
    const int nblk = (P + HEAD_TXT_PPB - 1) / HEAD_TXT_PPB;
    float* part = reinterpret_cast<float*>(ws);
    const size_t lds = ((size_t)(NB < RG ? NB : RG) * CH + KB * CH + 4 * PPW * CAP + 4 * PPW + 4 * CAP) * 4;
    constexpr int LDS_MAX = (RG * CH + KB * CH + 4 * PPW * CAP + 4 * PPW + 4 * CAP) * 4;      // 104.75 KiB
    const ProbeScope probe(EBC_PROBE_HEAD_BWD_TEXT, 0, 0, 0, 0, P, NB, CH, st);
    EBC_DTYPE_SWITCH(dtype_z,
        if (!ensure_lds<head_text_wide_bwd_kernel<T, CH>>(LDS_MAX, st)) return EBC_E_LAUNCH;
        hipLaunchKernelGGL((head_text_wide_bwd_kernel<T, CH>), dim3(nblk), dim3(256), lds, st, (const T*)Z, text, logit_scale,
                           anchors, dlogits, dexp, gscale, part, P, HW, NB));
    EBC_CHECK_LAUNCH();
    hipLaunchKernelGGL((head_text_finalize_kernel<CH, CAP>), dim3(CH / 64, NB), dim3(512), 0, st, part, nblk, NB, text,
                       logit_scale, dtext);
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

int head_bwd_text_wide(int dtype_z, const void* Z, const float* text, const float* logit_scale, const float* anchors,
                       const float* dlogits, const float* dexp, const float* gscale, float* dtext, int P, int HW, int NB,
                       int embed, void* ws, size_t wsb, hipStream_t st)
{
    if (NB <= 0 || NB > HEAD_MAX_BINS || (embed != 512 && embed != 1024)) return EBC_E_UNSUPPORTED;
    if (dtype_z != EBC_F32 && dtype_z != EBC_F16 && dtype_z != EBC_BF16) return EBC_E_ARG;
    if (!ws || wsb < head_bwd_text_wide_ws_bytes(P, NB, embed)) return EBC_E_ARG;
    if (embed == 512)
        return head_bwd_text_wide_t<512>(dtype_z, Z, text, logit_scale, anchors, dlogits, dexp, gscale, dtext, P, HW, NB, ws, st);
    return head_bwd_text_wide_t<1024>(dtype_z, Z, text, logit_scale, anchors, dlogits, dexp, gscale, dtext, P, HW, NB, ws, st);
}

int cast_f32(int dtype, const float* in, void* out, size_t n, hipStream_t st)
{
    if (n % 4) return EBC_E_ARG;
    EBC_DTYPE_SWITCH(dtype, hipLaunchKernelGGL(cast_kernel<T>, dim3(grid_for(n / 4)), dim3(256), 0, st, in, (T*)out, n / 4));
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

}  // namespace ebc
