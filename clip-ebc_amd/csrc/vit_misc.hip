// Memory-bound pieces of the CLIP-EBC ViT path on gfx950: LayerNorm fwd/bwd (with the deep-VPT prompt rows and
// their gradient), patch im2col, token embedding (+CLS, +pos, ln_pre, VPT rows), the prompt-gradient sum over crops
// and the f32 -> compute-dtype cast, with the C-ABI entry points of the single kernels.
//
// Reference: LayerNorm (fp32 math)        models/clip/_clip/blocks.py:8-14
//            token prologue               models/clip/model.py:147-158, image_encoder.py:141-148
//            VPT assemble / disassemble   models/clip/model.py:131-140, 161-183
//            ln_post + drop CLS           models/clip/model.py:185-188
// The row kernels are one wave per row (D = 256*NV), 16-B vector accesses, fp32 statistics.
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

int cast_f32(int dtype, const float* in, void* out, size_t n, hipStream_t st)
{
    if (n % 4) return EBC_E_ARG;
    EBC_DTYPE_SWITCH(dtype, hipLaunchKernelGGL(cast_kernel<T>, dim3(grid_for(n / 4)), dim3(256), 0, st, in, (T*)out, n / 4));
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

}  // namespace ebc

// ---------------------------------------------------------------------------- entry points
// Each validates on the host, before any device work (EBC_E_ARG), then goes to the launcher above, which the
// orchestrators (vit.hip, text.hip) call directly.
static bool ln_map_ok(int rpg, int gstride, int goff)
{
    return rpg <= 0 || (goff >= 0 && (long)goff + rpg <= (long)gstride);
}
extern "C" int ebc_layernorm_fwd(int dtype, const float* x, int rows_per_group, int group_stride, int group_offset,
                                 const float* gamma, const float* beta, void* out, float* out_f32, float* mean,
                                 float* rstd, int M, int D, ebc_stream_t stream)
{
    if (!x || !gamma || !beta || (!out && !out_f32) || (mean && !rstd)) return EBC_E_ARG;
    if (!ln_map_ok(rows_per_group, group_stride, group_offset)) return EBC_E_ARG;
    return ebc::layernorm_fwd(dtype, x, rows_per_group, group_stride, group_offset, gamma, beta, out, out_f32, mean,
                              rstd, M, D, (hipStream_t)stream);
}
extern "C" int ebc_layernorm_bwd(int dtype, int dy_f32, const void* dy, const float* x, int rows_per_group,
                                 int group_stride, int group_offset, const float* mean, const float* rstd,
                                 const float* gamma, const float* dx_in, float* dx_out, void* dx_out_t, int M, int D,
                                 ebc_stream_t stream)
{
    if (!dy || !x || !mean || !rstd || !gamma || !dx_out) return EBC_E_ARG;
    if (!ln_map_ok(rows_per_group, group_stride, group_offset)) return EBC_E_ARG;
    return ebc::layernorm_bwd(dtype, dy_f32, dy, x, rows_per_group, group_stride, group_offset, mean, rstd, gamma,
                              dx_in, dx_out, dx_out_t, M, D, (hipStream_t)stream);
}
extern "C" int ebc_im2col(int dtype, const float* x, void* out, int B, int H, int W, int patch, ebc_stream_t stream)
{
    if (!x || !out || B <= 0 || patch <= 0 || H < patch || W < patch) return EBC_E_ARG;
    return ebc::im2col(dtype, x, out, B, H, W, patch, (hipStream_t)stream);
}
extern "C" int ebc_cast_f32(int dtype, const float* in, void* out, size_t n, ebc_stream_t stream)
{
    if (!in || !out) return EBC_E_ARG;
    return ebc::cast_f32(dtype, in, out, n, (hipStream_t)stream);
}
