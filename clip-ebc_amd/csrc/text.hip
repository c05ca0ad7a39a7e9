// Kernels of a trained, causal CLIP text transformer on gfx950 (width 512, 8 heads of 64, up to 77 tokens):
// causal attention forward / backward, column sums (bias gradients), the LayerNorm parameter gradients, and the token +
// position embedding with its inverted-index backward.
//
// Reference: causal mask + attention     models/clip/_clip/text_encoder.py:33-39, blocks.py:35-37
//            embedding                   models/clip/_clip/text_encoder.py:42-44
//            LayerNorm parameters        models/clip/_clip/blocks.py:8-14
// No float atomics anywhere: every sum runs in a fixed order, so two launches on the same inputs agree bit for bit.
#include <algorithm>

#include "ebc_common.h"
#include "kernels.h"
#include "mfma.h"
#include "vec_io.h"

using namespace ebc;

namespace {

// ---------------------------------------------------------------------------------------- causal attention
// One workgroup per (prompt, head), five waves: wave w owns query tile w (16 rows) and, in the backward, key tile w.
// Q, K, V (and dO) of the ceil(L / 16) tiles sit in LDS, rows >= L zero.  Key tiles above the diagonal are never
// touched; the diagonal tile is masked per element, which also masks the ragged tile's keys >= L (key > query there).
constexpr int CA_HD = 64;
constexpr int CA_LMAX = 77;
constexpr int CA_ROWS = 80;          // 5 tiles
constexpr int CA_THREADS = 320;
constexpr int CA_PLD = 88;           // row stride of the P / dS matrices (elements)
constexpr float CA_C2 = 0.18033688011112042f;     // log2(e) / 8
constexpr float CA_LOG2E = 1.4426950408889634f;
template <class E> constexpr int ca_ld() { return E::BYTES == 4 ? 68 : 72; }      // row stride of Q / K / V / dO
template <class E> constexpr int ca_fwd_lds() { return (3 * CA_ROWS * ca_ld<E>() + CA_ROWS * CA_PLD) * E::BYTES; }
template <class E> constexpr int ca_bwd_lds()
{
    return (4 * CA_ROWS * ca_ld<E>() + 2 * CA_ROWS * CA_PLD) * E::BYTES + 2 * CA_ROWS * (int)sizeof(float);
}

extern __shared__ __attribute__((aligned(16))) unsigned char ca_smem[];

template <class T> __device__ __forceinline__ void copy8(T* dst, const T* src)
{
#pragma unroll
    for (int i = 0; i < (int)sizeof(T) / 2; ++i) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
}
template <class T> __device__ __forceinline__ void zero8(T* dst)
{
#pragma unroll
    for (int i = 0; i < (int)sizeof(T) / 2; ++i) reinterpret_cast<uint4*>(dst)[i] = make_uint4(0, 0, 0, 0);
}

// rows [0, rows) of one [L][64] operand (global row stride ldg) -> LDS [rows][LD], rows >= L zero
template <class T, int LD>
__device__ __forceinline__ void ca_stage(T* lds, const T* g, size_t ldg, int L, int rows)
{
    for (int idx = threadIdx.x; idx < rows * 8; idx += CA_THREADS) {
        const int r = idx >> 3, ch = idx & 7;
        if (r < L) copy8<T>(lds + r * LD + 8 * ch, g + (size_t)r * ldg + 8 * ch);
        else zero8<T>(lds + r * LD + 8 * ch);
    }
}

// Operand of a product over the head dim: X[row0 + (l & 15)][k0 + 8 (l >> 4) + j], both operands alike
template <class E>
__device__ __forceinline__ typename E::Frag rowfrag(const typename E::T* lds, int ld, int row0, int k0)
{
    const int l = threadIdx.x & 63;
    return load8<E>(lds + (row0 + (l & 15)) * ld + k0 + 8 * (l >> 4));
}

// Operands of a product over tokens, 32 (full) or 16 at a time.  Both carry mfma.h load_colfrag's k order: element j of
// lane l is token r0 + 4 (l >> 4) + j for j < 4 and r0 + 16 + 4 (l >> 4) + (j - 4) above; the upper half is zero when
// the step holds one tile only.
// colfrag: X[token][n0 + (l & 15)] of a row-major [token][.] matrix
template <class E>
__device__ __forceinline__ typename E::Frag colfrag(const typename E::T* lds, int ld, int r0, int n0, bool full);
template <> __device__ __forceinline__ f32x8 colfrag<EF32>(const float* lds, int ld, int r0, int n0, bool full)
{
    const int l = threadIdx.x & 63, g = l >> 4, c = n0 + (l & 15);
    f32x8 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        r[j] = lds[(r0 + 4 * g + j) * ld + c];
        r[j + 4] = full ? lds[(r0 + 16 + 4 * g + j) * ld + c] : 0.f;
    }
    return r;
}
template <class E16>
__device__ __forceinline__ typename E16::Frag colfrag16(const typename E16::T* lds, int ld, int r0, int n0, bool full)
{
    const int l = threadIdx.x & 63, g = l >> 4, w = l & 15, q = w >> 2, p = w & 3;
    const typename E16::T* a0 = lds + (r0 + 4 * g + q) * ld + n0 + 4 * p;
    // the transposed read gathers across lanes and needs every lane active: both halves are always issued (the upper
    // one on the lower block's address when there is no second tile) and the unused half is cleared afterwards
    const typename E16::T* a1 = full ? a0 + 16 * ld : a0;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a1));
    if (!full) hi = s16x4{0, 0, 0, 0};
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(typename E16::Frag, v);
}
template <> __device__ __forceinline__ f16x8 colfrag<EF16>(const _Float16* lds, int ld, int r0, int n0, bool full)
{
    return colfrag16<EF16>(lds, ld, r0, n0, full);
}
template <> __device__ __forceinline__ bf16x8 colfrag<EBF16>(const __bf16* lds, int ld, int r0, int n0, bool full)
{
    return colfrag16<EBF16>(lds, ld, r0, n0, full);
}
// permfrag: X[row0 + (l & 15)][token] of a row-major [.][token] matrix (P or dS as the A operand)
template <class E>
__device__ __forceinline__ typename E::Frag permfrag(const typename E::T* lds, int ld, int row0, int k0, bool full)
{
    using T = typename E::T;
    const int l = threadIdx.x & 63;
    const T* p = lds + (row0 + (l & 15)) * ld + k0 + 4 * (l >> 4);
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    ld4<T>(p, v);
    if (full) ld4<T>(p + 16, v + 4);
    return pack8<E>(v);
}

__device__ __forceinline__ float row16_max(float v)
{
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float row16_sum(float v)
{
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// out [B*L][H*64] = softmax(q k^T / 8 over keys <= query) v, lse [B][H][L] = log sum exp of the scaled scores
template <class E>
__global__ __launch_bounds__(CA_THREADS) void attn_causal_fwd_kernel(const typename E::T* __restrict__ qkv,
                                                                     typename E::T* __restrict__ out,
                                                                     float* __restrict__ lse, int L, int H)
{
    using T = typename E::T;
    constexpr int LD = ca_ld<E>();
    T* Qs = reinterpret_cast<T*>(ca_smem);
    T* Ks = Qs + CA_ROWS * LD;
    T* Vs = Ks + CA_ROWS * LD;
    T* Ps = Vs + CA_ROWS * LD;                       // [CA_ROWS][CA_PLD], each wave its own 16 rows
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int i = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);         // the wave: scalar, so its branches are too
    const int l = threadIdx.x & 63, g = l >> 4, c = l & 15;
    const int nt = (L + 15) >> 4, rows = 16 * nt;
    const size_t ldg = (size_t)3 * H * CA_HD;
    const T* base = qkv + (size_t)b * L * ldg + (size_t)h * CA_HD;
    ca_stage<T, LD>(Qs, base, ldg, L, rows);
    ca_stage<T, LD>(Ks, base + (size_t)H * CA_HD, ldg, L, rows);
    ca_stage<T, LD>(Vs, base + (size_t)2 * H * CA_HD, ldg, L, rows);
    __syncthreads();
    const bool act = i < nt;                         // wave-uniform
    float mrow[4], srow[4];
    if (act) {
        f32x4 s[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (j <= i) {
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
                    s[j] = mma(rowfrag<E>(Qs, LD, 16 * i, 32 * kk), rowfrag<E>(Ks, LD, 16 * j, 32 * kk), s[j]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * i + 4 * g + r;
            float m = -INFINITY;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                if (j <= i) {
                    if (16 * j + c > row) s[j][r] = -INFINITY;
                    m = fmaxf(m, s[j][r]);
                }
            }
            m = row16_max(m);                        // finite: the diagonal is never masked
            const float mc = m * CA_C2;
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                if (j <= i) {
                    const float p = exp2f(fmaf(s[j][r], CA_C2, -mc));       // masked: exp2(-inf) = 0
                    sum += p;
                    Ps[row * CA_PLD + 16 * j + c] = E::from(p);
                }
            }
            mrow[r] = m;
            srow[r] = row16_sum(sum);
        }
    }
    __syncthreads();
    if (!act) return;
    f32x4 o[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kend = 16 * (i + 1);
    for (int k0 = 0; k0 < kend; k0 += 32) {
        const bool full = k0 + 16 < kend;
        const typename E::Frag a = permfrag<E>(Ps, CA_PLD, 16 * i, k0, full);
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) o[nb] = mma(a, colfrag<E>(Vs, LD, k0, 16 * nb, full), o[nb]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * i + 4 * g + r;
        if (row >= L) continue;
        const float inv = 1.0f / srow[r];
        T* orow = out + ((size_t)b * L + row) * H * CA_HD + (size_t)h * CA_HD;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) orow[16 * nb + c] = E::from(o[nb][r] * inv);
        if (lse && c == 0) lse[((size_t)b * H + h) * L + row] = mrow[r] * 0.125f + logf(srow[r]);
    }
}

// dqkv [B*L][3*H*64] from P = exp(s - lse) on keys <= query, delta = rowsum(dout * out), dS = P (dP - delta):
// dQ = dS K / 8, dK = dS^T Q / 8, dV = P^T dO.  Phase 1: wave i writes its rows of P and dS to LDS; phase 2: wave i
// forms dQ of query tile i and (transposed, so P and dS are read as stored) dK and dV of key tile i.
template <class E>
__global__ __launch_bounds__(CA_THREADS) void attn_causal_bwd_kernel(const typename E::T* __restrict__ qkv,
                                                                     const typename E::T* __restrict__ dout,
                                                                     const typename E::T* __restrict__ out,
                                                                     const float* __restrict__ lse,
                                                                     typename E::T* __restrict__ dqkv, int L, int H)
{
    using T = typename E::T;
    constexpr int LD = ca_ld<E>();
    T* Qs = reinterpret_cast<T*>(ca_smem);
    T* Ks = Qs + CA_ROWS * LD;
    T* Vs = Ks + CA_ROWS * LD;
    T* Ds = Vs + CA_ROWS * LD;
    T* Pm = Ds + CA_ROWS * LD;                       // [CA_ROWS][CA_PLD]
    T* Sm = Pm + CA_ROWS * CA_PLD;
    float* lse_s = reinterpret_cast<float*>(Sm + CA_ROWS * CA_PLD);      // lse * log2(e)
    float* delta_s = lse_s + CA_ROWS;
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int i = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);         // the wave: scalar, so its branches are too
    const int l = threadIdx.x & 63, g = l >> 4, c = l & 15;
    const int nt = (L + 15) >> 4, rows = 16 * nt;
    const size_t ldg = (size_t)3 * H * CA_HD, ldo = (size_t)H * CA_HD;
    const T* base = qkv + (size_t)b * L * ldg + (size_t)h * CA_HD;
    const T* dobase = dout + (size_t)b * L * ldo + (size_t)h * CA_HD;
    ca_stage<T, LD>(Qs, base, ldg, L, rows);
    ca_stage<T, LD>(Ks, base + (size_t)H * CA_HD, ldg, L, rows);
    ca_stage<T, LD>(Vs, base + (size_t)2 * H * CA_HD, ldg, L, rows);
    ca_stage<T, LD>(Ds, dobase, ldo, L, rows);
    if ((int)threadIdx.x < rows) {
        const int r = threadIdx.x;
        float d = 0.f, ls = 0.f;
        if (r < L) {
            const T* orow = out + ((size_t)b * L + r) * ldo + (size_t)h * CA_HD;
            for (int ch = 0; ch < 8; ++ch) {
                float a[8], o8[8];
                ld4<T>(dobase + (size_t)r * ldo + 8 * ch, a);
                ld4<T>(dobase + (size_t)r * ldo + 8 * ch + 4, a + 4);
                ld4<T>(orow + 8 * ch, o8);
                ld4<T>(orow + 8 * ch + 4, o8 + 4);
#pragma unroll
                for (int e = 0; e < 8; ++e) d += a[e] * o8[e];
            }
            ls = lse[((size_t)b * H + h) * L + r] * CA_LOG2E;
        }
        delta_s[r] = d;
        lse_s[r] = ls;
    }
    __syncthreads();
    const bool act = i < nt;                         // wave-uniform
    if (act) {
        for (int j = 0; j <= i; ++j) {
            f32x4 sa = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                sa = mma(rowfrag<E>(Qs, LD, 16 * i, 32 * kk), rowfrag<E>(Ks, LD, 16 * j, 32 * kk), sa);
                dp = mma(rowfrag<E>(Ds, LD, 16 * i, 32 * kk), rowfrag<E>(Vs, LD, 16 * j, 32 * kk), dp);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * i + 4 * g + r, col = 16 * j + c;
                float p = 0.f, ds = 0.f;
                if (col <= row && row < L) {
                    p = exp2f(fmaf(sa[r], CA_C2, -lse_s[row]));
                    ds = p * (dp[r] - delta_s[row]);
                }
                Pm[row * CA_PLD + col] = E::from(p);
                Sm[row * CA_PLD + col] = E::from(ds);
            }
        }
    }
    __syncthreads();
    if (!act) return;
    T* gbase = dqkv + (size_t)b * L * ldg + (size_t)h * CA_HD;
    {   // dQ of query tile i: keys 0 .. 16 (i + 1)
        f32x4 dq[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) dq[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kend = 16 * (i + 1);
        for (int k0 = 0; k0 < kend; k0 += 32) {
            const bool full = k0 + 16 < kend;
            const typename E::Frag a = permfrag<E>(Sm, CA_PLD, 16 * i, k0, full);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) dq[nb] = mma(a, colfrag<E>(Ks, LD, k0, 16 * nb, full), dq[nb]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * i + 4 * g + r;
            if (row >= L) continue;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) gbase[(size_t)row * ldg + 16 * nb + c] = E::from(dq[nb][r] * 0.125f);
        }
    }
    {   // dK^T, dV^T [d][key] of key tile i: queries 16 i .. rows
        f32x4 dk[4], dv[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) { dk[nb] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[nb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        for (int q0 = 16 * i; q0 < rows; q0 += 32) {
            const bool full = q0 + 16 < rows;
            const typename E::Frag bs = colfrag<E>(Sm, CA_PLD, q0, 16 * i, full);
            const typename E::Frag bp = colfrag<E>(Pm, CA_PLD, q0, 16 * i, full);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                dk[nb] = mma(colfrag<E>(Qs, LD, q0, 16 * nb, full), bs, dk[nb]);
                dv[nb] = mma(colfrag<E>(Ds, LD, q0, 16 * nb, full), bp, dv[nb]);
            }
        }
        const int key = 16 * i + c;
        if (key < L) {
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                const float4 k4 = make_float4(dk[nb][0] * 0.125f, dk[nb][1] * 0.125f, dk[nb][2] * 0.125f, dk[nb][3] * 0.125f);
                const float4 v4 = make_float4(dv[nb][0], dv[nb][1], dv[nb][2], dv[nb][3]);
                st4<T>(gbase + (size_t)key * ldg + (size_t)H * CA_HD + 16 * nb + 4 * g, k4);
                st4<T>(gbase + (size_t)key * ldg + (size_t)2 * H * CA_HD + 16 * nb + 4 * g, v4);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------- column sums
// out[c] = sum_r a[r][c] over [M][N]; XHAT: also out2[c] = sum_r a[r][c] xhat[r][c], xhat = (x - mean[r]) rstd[r] (the
// LayerNorm parameter gradients: out = d beta, out2 = d gamma).  A block takes 32 columns; its eight row groups each sum
// the rows r = group (mod 8) in ascending order, then thread 0..31 adds the eight partials in group order.
template <class TA, bool XHAT>
__global__ __launch_bounds__(256) void colsum_kernel(const TA* __restrict__ a, const float* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     float* __restrict__ out, float* __restrict__ out2, int M, int N)
{
    __shared__ float part[2][8][32];
    const int cl = threadIdx.x & 31, rg = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    float s = 0.f, s2 = 0.f;
    if (c < N) {
        for (int r = rg; r < M; r += 8) {
            const float v = (float)a[(size_t)r * N + c];
            s += v;
            if constexpr (XHAT) s2 += v * ((x[(size_t)r * N + c] - mean[r]) * rstd[r]);
        }
    }
    part[0][rg][cl] = s;
    part[1][rg][cl] = s2;
    __syncthreads();
    if (rg == 0 && c < N) {
        float t = part[0][0][cl], t2 = part[1][0][cl];
#pragma unroll
        for (int k = 1; k < 8; ++k) { t += part[0][k][cl]; t2 += part[1][k][cl]; }
        out[c] = t;
        if constexpr (XHAT) out2[c] = t2;
    }
}

// ---------------------------------------------------------------------------------------- embedding
constexpr int TX_D = 512;

// x[r] = token_embedding[ids[r]] + positional_embedding[r % Lt], one wave a row; an id outside the table reads as zero
__global__ __launch_bounds__(256) void text_embed_fwd_kernel(const float* __restrict__ tok, const float* __restrict__ pos,
                                                             const int* __restrict__ ids, float* __restrict__ X, int M,
                                                             int Lt, int vocab)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const int id = ids[r], t = r % Lt;
    const bool ok = id >= 0 && id < vocab;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = 4 * lane + 256 * i;
        const float4 a = ok ? *reinterpret_cast<const float4*>(tok + (size_t)id * TX_D + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 p = *reinterpret_cast<const float4*>(pos + (size_t)t * TX_D + c);
        *reinterpret_cast<float4*>(X + (size_t)r * TX_D + c) = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
    }
}

// One wave per destination row, every row written: token row v (< vocab) is the sum of the dx rows of its list
// rows[offs[u] .. offs[u + 1]) in list order when v = uniq[u] (uniq ascending, found by bisection), else zero;
// position row t is sum_p dx[p][t] in prompt order for t < Lt, else zero.
__global__ __launch_bounds__(256) void text_embed_bwd_kernel(const float* __restrict__ dX, const int* __restrict__ uniq,
                                                             const int* __restrict__ offs, const int* __restrict__ rows,
                                                             int nu, float* __restrict__ dtok, float* __restrict__ dpos,
                                                             int NB, int Lt, int ctx, int vocab)
{
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, M = NB * Lt;
    if (row >= (long)vocab + ctx) return;
    float4 acc[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    float* dst;
    if (row < vocab) {
        dst = dtok + (size_t)row * TX_D;
        int lo = 0, hi = nu;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (uniq[mid] < (int)row) lo = mid + 1; else hi = mid;
        }
        if (lo < nu && uniq[lo] == (int)row) {
            const int e0 = max(offs[lo], 0), e1 = min(offs[lo + 1], M);
            for (int e = e0; e < e1; ++e) {
                const int r = rows[e];
                if ((unsigned)r >= (unsigned)M) continue;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const float4 v = *reinterpret_cast<const float4*>(dX + (size_t)r * TX_D + 4 * lane + 256 * i);
                    acc[i].x += v.x; acc[i].y += v.y; acc[i].z += v.z; acc[i].w += v.w;
                }
            }
        }
    } else {
        const int t = (int)(row - vocab);
        dst = dpos + (size_t)t * TX_D;
        if (t < Lt) {
            for (int p = 0; p < NB; ++p) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const float4 v = *reinterpret_cast<const float4*>(dX + ((size_t)p * Lt + t) * TX_D + 4 * lane + 256 * i);
                    acc[i].x += v.x; acc[i].y += v.y; acc[i].z += v.z; acc[i].w += v.w;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(dst + 4 * lane + 256 * i) = acc[i];
}

template <class TA>
int colsum_launch(const void* a, const float* x, const float* mean, const float* rstd, float* out, float* out2, int M,
                  int N, hipStream_t st)
{
    const dim3 grid((N + 31) / 32);
    if (x)
        hipLaunchKernelGGL((colsum_kernel<TA, true>), grid, dim3(256), 0, st, (const TA*)a, x, mean, rstd, out, out2, M, N);
    else
        hipLaunchKernelGGL((colsum_kernel<TA, false>), grid, dim3(256), 0, st, (const TA*)a, x, mean, rstd, out, out2, M, N);
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- C-ABI
extern "C" int ebc_attention_causal_fwd(int dtype, const void* qkv, void* out, float* lse, int B, int L, int H,
                                        ebc_stream_t stream)
{
    if (!qkv || !out || B <= 0 || H <= 0 || L <= 0) return EBC_E_ARG;
    if (dtype != EBC_F32 && dtype != EBC_F16 && dtype != EBC_BF16) return EBC_E_ARG;
    if (L > CA_LMAX) return EBC_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    EBC_DTYPE_SWITCH(dtype, {
        constexpr int bytes = ca_fwd_lds<E>();
        if (!ensure_lds<attn_causal_fwd_kernel<E>>(bytes, st)) return EBC_E_LAUNCH;
        hipLaunchKernelGGL(attn_causal_fwd_kernel<E>, dim3(B * H), dim3(CA_THREADS), bytes, st, (const T*)qkv, (T*)out, lse,
                           L, H);
    });
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

extern "C" int ebc_attention_causal_bwd(int dtype, const void* qkv, const void* dout, const void* out, const float* lse,
                                        float* delta_ws, void* dqkv, int B, int L, int H, ebc_stream_t stream)
{
    (void)delta_ws;                                  // delta stays in LDS at every dtype
    if (!qkv || !dout || !out || !lse || !dqkv || B <= 0 || H <= 0 || L <= 0) return EBC_E_ARG;
    if (dtype != EBC_F32 && dtype != EBC_F16 && dtype != EBC_BF16) return EBC_E_ARG;
    if (L > CA_LMAX) return EBC_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    EBC_DTYPE_SWITCH(dtype, {
        constexpr int bytes = ca_bwd_lds<E>();
        if (!ensure_lds<attn_causal_bwd_kernel<E>>(bytes, st)) return EBC_E_LAUNCH;
        hipLaunchKernelGGL(attn_causal_bwd_kernel<E>, dim3(B * H), dim3(CA_THREADS), bytes, st, (const T*)qkv,
                           (const T*)dout, (const T*)out, lse, (T*)dqkv, L, H);
    });
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

extern "C" int ebc_colsum(int dtype, int in_f32, const void* a, float* out, int M, int N, ebc_stream_t stream)
{
    if (!a || !out || M <= 0 || N <= 0) return EBC_E_ARG;
    if (dtype != EBC_F32 && dtype != EBC_F16 && dtype != EBC_BF16) return EBC_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (in_f32) return colsum_launch<float>(a, nullptr, nullptr, nullptr, out, nullptr, M, N, st);
    EBC_DTYPE_SWITCH(dtype, return colsum_launch<T>(a, nullptr, nullptr, nullptr, out, nullptr, M, N, st));
    return EBC_OK;
}

extern "C" int ebc_layernorm_param_grad(int dtype, int dy_f32, const void* dy, const float* x, const float* mean,
                                        const float* rstd, float* dgamma, float* dbeta, int M, int D,
                                        ebc_stream_t stream)
{
    if (!dy || !x || !mean || !rstd || !dgamma || !dbeta || M <= 0) return EBC_E_ARG;
    if (dtype != EBC_F32 && dtype != EBC_F16 && dtype != EBC_BF16) return EBC_E_ARG;
    if (D != 512 && D != 768) return EBC_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (dy_f32) return colsum_launch<float>(dy, x, mean, rstd, dbeta, dgamma, M, D, st);
    EBC_DTYPE_SWITCH(dtype, return colsum_launch<T>(dy, x, mean, rstd, dbeta, dgamma, M, D, st));
    return EBC_OK;
}

static int text_embed_args(int NB, int Lt, int width)
{
    if (NB < 1 || NB > 16 || Lt < 1 || Lt > CA_LMAX || width != TX_D) return EBC_E_UNSUPPORTED;
    return EBC_OK;
}

extern "C" int ebc_text_embed_fwd(const float* token_embedding, const float* positional_embedding, const int* ids, float* x,
                                  int NB, int Lt, int width, int vocab, ebc_stream_t stream)
{
    if (!token_embedding || !positional_embedding || !ids || !x || vocab <= 0) return EBC_E_ARG;
    EBC_TRY(text_embed_args(NB, Lt, width));
    const int M = NB * Lt;
    hipLaunchKernelGGL(text_embed_fwd_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, token_embedding,
                       positional_embedding, ids, x, M, Lt, vocab);
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

extern "C" int ebc_text_embed_bwd(const float* dx, const int* uniq, const int* offs, const int* rows, int nu, float* dtoken,
                                  float* dpos, int NB, int Lt, int context, int width, int vocab, ebc_stream_t stream)
{
    if (!dx || !uniq || !offs || !rows || !dtoken || !dpos || vocab <= 0) return EBC_E_ARG;
    EBC_TRY(text_embed_args(NB, Lt, width));
    if (context < Lt || context > CA_LMAX || nu < 1 || nu > NB * Lt) return EBC_E_ARG;
    const long total = (long)vocab + context;
    hipLaunchKernelGGL(text_embed_bwd_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dx, uniq,
                       offs, rows, nu, dtoken, dpos, NB, Lt, context, vocab);
    EBC_CHECK_LAUNCH();
    return EBC_OK;
}

// ---------------------------------------------------------------------------------------------- the tower
// Host-side sequencing of the text transformer (text_encoder.py:41-53 over blocks.py:22-42), forward and the backward of
// every parameter.  Layout in the workspace (M = NB * Lt rows, row-major [NB][Lt][512]):
//   per layer   the compute-dtype weights [out][in] and their transposes (made by every forward: the weights train)
//   X_l f32     residual stream entering block l; X1_l after the attention half; mean / rstd of ln_1, ln_2
//   H1_l, H2_l  T [M,512] LayerNorm outputs (weight-gradient operands); QKV_l T [M,1536]; O_l T [M,512]; lse_l
//   A_l, G_l    T [M,2048] MLP pre-activation and QuickGELU output
// Weight gradients are ebc_gemm_wgrad products over the rows: both operands transposed to [channels][Mp], Mp = M rounded
// up to 64, the padding columns zeroed by one memset a backward.
namespace {

constexpr int TW = 512, THEADS = 8, TMLP = 2048, TQKV = 3 * TW;
constexpr size_t WGRAD_CNT_BYTES = 16 * 1024;

struct TLayerW { void *qkv, *qkv_t, *out, *out_t, *fc, *fc_t, *proj, *proj_t; };
struct TLayerSave {
    float *X1, *m1, *r1, *m2, *r2, *lse;
    void *H1, *QKV, *O, *H2, *A, *G;
};
struct TLayout {
    TLayerW w[64];
    TLayerSave s[64];
    float* X[65];
    void *tproj, *tproj_t;              // text_projection [512][embed] and its transpose [embed][512]
    float *Xe, *mf, *rf;                // EOT rows of X_layers [NB][512] and ln_final's statistics
    void* He;                           // ln_final output T [NB][512]
    // backward
    float *dXa, *dXb, *dXe;
    void *dXt, *dH, *dA, *dO, *dQKV, *dFt, *dHe;
    char* zero0;                        // start of the region one memset clears: the transposed operands + wgrad counters
    void *tA, *tB, *tE1, *tE2, *wg;
    size_t zero_bytes, wg_bytes;
    int Mp;
    size_t bytes;
};

size_t wgrad_ws_max(int dtype, int Mp, int embed)
{
    size_t b = 0;
    const int shapes[5][3] = {{TW, TMLP, Mp}, {TMLP, TW, Mp}, {TW, TW, Mp}, {TQKV, TW, Mp}, {TW, embed, 64}};
    for (const auto& s : shapes) b = std::max(b, ebc_gemm_wgrad_workspace_bytes(dtype, s[0], s[1], s[2]));
    return std::max(b, WGRAD_CNT_BYTES);
}

TLayout text_carve(void* ws, int NB, int Lt, int layers, int embed, int dtype, int training)
{
    const size_t M = (size_t)NB * Lt, es = dtype == EBC_F32 ? 4 : 2;
    Carver c{(char*)ws};
    TLayout lay{};
    lay.Mp = (int)((M + 63) / 64 * 64);
    const int nsave = training ? layers : 1;
    for (int l = 0; l < layers; ++l) {
        if (l >= nsave) { lay.w[l] = lay.w[0]; lay.s[l] = lay.s[0]; continue; }
        TLayerW& w = lay.w[l];
        w.qkv = c.take<void>((size_t)TQKV * TW * es);   w.qkv_t = c.take<void>((size_t)TQKV * TW * es);
        w.out = c.take<void>((size_t)TW * TW * es);     w.out_t = c.take<void>((size_t)TW * TW * es);
        w.fc = c.take<void>((size_t)TMLP * TW * es);    w.fc_t = c.take<void>((size_t)TMLP * TW * es);
        w.proj = c.take<void>((size_t)TW * TMLP * es);  w.proj_t = c.take<void>((size_t)TW * TMLP * es);
        TLayerSave& s = lay.s[l];
        s.X1 = c.take<float>(M * TW * 4);
        s.m1 = c.take<float>(M * 4); s.r1 = c.take<float>(M * 4);
        s.m2 = c.take<float>(M * 4); s.r2 = c.take<float>(M * 4);
        s.lse = c.take<float>((size_t)NB * THEADS * Lt * 4);
        s.H1 = c.take<void>(M * TW * es);
        s.QKV = c.take<void>(M * TQKV * es);
        s.O = c.take<void>(M * TW * es);
        s.H2 = c.take<void>(M * TW * es);
        s.A = c.take<void>(M * TMLP * es);
        s.G = c.take<void>(M * TMLP * es);
    }
    for (int l = 0; l <= layers; ++l) lay.X[l] = (training || l < 2) ? c.take<float>(M * TW * 4) : lay.X[l & 1];
    lay.tproj = c.take<void>((size_t)TW * embed * es);
    lay.tproj_t = c.take<void>((size_t)TW * embed * es);
    lay.Xe = c.take<float>((size_t)NB * TW * 4);
    lay.mf = c.take<float>((size_t)NB * 4);
    lay.rf = c.take<float>((size_t)NB * 4);
    lay.He = c.take<void>((size_t)NB * TW * es);
    if (training) {
        lay.dXa = c.take<float>(M * TW * 4);
        lay.dXb = c.take<float>(M * TW * 4);
        lay.dXe = c.take<float>((size_t)NB * TW * 4);
        lay.dXt = c.take<void>(M * TW * es);
        lay.dH = c.take<void>(M * TW * es);
        lay.dA = c.take<void>(M * TMLP * es);
        lay.dO = c.take<void>(M * TW * es);
        lay.dQKV = c.take<void>(M * TQKV * es);
        lay.dFt = c.take<void>((size_t)NB * embed * es);
        lay.dHe = c.take<void>((size_t)NB * TW * es);
        const size_t z0 = c.off;
        lay.zero0 = ws ? (char*)ws + z0 : nullptr;
        lay.tA = c.take<void>((size_t)TMLP * lay.Mp * es);
        lay.tB = c.take<void>((size_t)TMLP * lay.Mp * es);
        lay.tE1 = c.take<void>((size_t)TW * 64 * es);
        lay.tE2 = c.take<void>((size_t)embed * 64 * es);
        lay.wg_bytes = wgrad_ws_max(dtype, lay.Mp, embed);
        lay.wg = c.take<void>(WGRAD_CNT_BYTES);                       // the counter block is cleared, the rest is scratch
        lay.zero_bytes = c.off - z0;
        if (lay.wg_bytes > WGRAD_CNT_BYTES) c.take<void>(lay.wg_bytes - WGRAD_CNT_BYTES);
    }
    lay.bytes = c.off;
    return lay;
}

int text_dims(int NB, int Lt, int embed)
{
    if (NB < 1 || NB > 16 || Lt < 1 || Lt > CA_LMAX || (embed != 512 && embed != 1024)) return EBC_E_UNSUPPORTED;
    return EBC_OK;
}
bool text_dtype_ok(int dtype) { return dtype == EBC_F32 || dtype == EBC_F16 || dtype == EBC_BF16; }

bool text_layer_ok(const EbcTextLayer& p)
{
    return p.w_qkv && p.b_qkv && p.w_out && p.b_out && p.w_fc && p.b_fc && p.w_proj && p.b_proj && p.ln1_g && p.ln1_b &&
           p.ln2_g && p.ln2_b;
}
bool text_layer_ok(const EbcTextLayerGrads& p)
{
    return p.w_qkv && p.b_qkv && p.w_out && p.b_out && p.w_fc && p.b_fc && p.w_proj && p.b_proj && p.ln1_g && p.ln1_b &&
           p.ln2_g && p.ln2_b;
}
// EBC_E_ARG / EBC_E_UNSUPPORTED of a weights struct (the dimension rules first, as the workspace size answers them)
int text_weights_check(const EbcTextWeights* w, int NB, int Lt, int dtype)
{
    if (!w || !w->layer || w->layers <= 0 || w->layers > 64 || !text_dtype_ok(dtype)) return EBC_E_ARG;
    if (w->width != TW) return EBC_E_UNSUPPORTED;
    EBC_TRY(text_dims(NB, Lt, w->embed));
    if (w->heads != THEADS || w->vocab <= 0 || w->context < Lt || w->context > CA_LMAX) return EBC_E_ARG;
    if (!w->token_embedding || !w->positional_embedding || !w->ln_final_g || !w->ln_final_b || !w->text_projection)
        return EBC_E_ARG;
    for (int l = 0; l < w->layers; ++l)
        if (!text_layer_ok(w->layer[l])) return EBC_E_ARG;
    return EBC_OK;
}

// xe[k] = X[k * Lt + eot[k]] (an eot outside the prompt reads row Lt - 1)
__global__ __launch_bounds__(256) void text_eot_gather_kernel(const float* __restrict__ X, const int* __restrict__ eot,
                                                              float* __restrict__ xe, int NB, int Lt)
{
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= NB) return;
    const int t = min(max(eot[k], 0), Lt - 1);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = 4 * lane + 256 * i;
        *reinterpret_cast<float4*>(xe + (size_t)k * TX_D + c) =
            *reinterpret_cast<const float4*>(X + ((size_t)k * Lt + t) * TX_D + c);
    }
}

// The adjoint: dX [NB*Lt][512] f32 and its compute-dtype copy, row (k, eot[k]) = dxe[k], every other row zero
template <class T>
__global__ __launch_bounds__(256) void text_eot_scatter_kernel(const float* __restrict__ dxe, const int* __restrict__ eot,
                                                               float* __restrict__ dX, T* __restrict__ dXt, int NB, int Lt)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= NB * Lt) return;
    const int k = r / Lt, t = r - k * Lt;
    const bool hit = t == min(max(eot[k], 0), Lt - 1);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = 4 * lane + 256 * i;
        const float4 v = hit ? *reinterpret_cast<const float4*>(dxe + (size_t)k * TX_D + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(dX + (size_t)r * TX_D + c) = v;
        st4<T>(dXt + (size_t)r * TX_D + c, v);
    }
}

}  // namespace

extern "C" size_t ebc_text_workspace_bytes(int NB, int Lt, int layers, int embed, int dtype, int training)
{
    if (text_dims(NB, Lt, embed) != EBC_OK || layers <= 0 || layers > 64 || !text_dtype_ok(dtype)) return 0;
    return text_carve(nullptr, NB, Lt, layers, embed, dtype, training).bytes;
}

extern "C" int ebc_text_forward(const EbcTextWeights* w, const int* ids, const int* eot, int NB, int Lt, int dtype,
                                int training, void* ws, size_t wsb, float* features, ebc_stream_t stream)
{
    EBC_TRY(text_weights_check(w, NB, Lt, dtype));
    if (!ids || !eot || !ws || !features) return EBC_E_ARG;
    const int layers = w->layers, embed = w->embed, M = NB * Lt;
    const TLayout lay = text_carve(ws, NB, Lt, layers, embed, dtype, training);
    if (lay.bytes > wsb) return EBC_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    auto gemm = [&](int epi, int out_f32, const void* A, const void* Bm, void* C, const float* bias, const float* resid,
                    void* aux, int m, int n, int k) {
        return ebc::gemm_nt(dtype, epi, out_f32, A, Bm, C, bias, resid, aux, m, n, k, st);
    };
    EBC_TRY(ebc_text_embed_fwd(w->token_embedding, w->positional_embedding, ids, lay.X[0], NB, Lt, TW, w->vocab, stream));
    for (int l = 0; l < layers; ++l) {
        const EbcTextLayer& p = w->layer[l];
        const TLayerW& c = lay.w[l];
        const TLayerSave& s = lay.s[l];
        EBC_TRY(ebc_prep_weights_1x1(dtype, p.w_qkv, c.qkv, c.qkv_t, TQKV, TW, stream));
        EBC_TRY(ebc_prep_weights_1x1(dtype, p.w_out, c.out, c.out_t, TW, TW, stream));
        EBC_TRY(ebc_prep_weights_1x1(dtype, p.w_fc, c.fc, c.fc_t, TMLP, TW, stream));
        EBC_TRY(ebc_prep_weights_1x1(dtype, p.w_proj, c.proj, c.proj_t, TW, TMLP, stream));
        // x = x + out_proj(attn(ln_1(x)))  (blocks.py:35-40)
        EBC_TRY(ebc::layernorm_fwd(dtype, lay.X[l], 0, 0, 0, p.ln1_g, p.ln1_b, s.H1, nullptr, s.m1, s.r1, M, TW, st));
        EBC_TRY(gemm(EBC_EPI_STORE, 0, s.H1, c.qkv, s.QKV, p.b_qkv, nullptr, nullptr, M, TQKV, TW));
        EBC_TRY(ebc_attention_causal_fwd(dtype, s.QKV, s.O, s.lse, NB, Lt, THEADS, stream));
        EBC_TRY(gemm(EBC_EPI_RESID, 1, s.O, c.out, s.X1, p.b_out, lay.X[l], nullptr, M, TW, TW));
        // x = x + c_proj(QuickGELU(c_fc(ln_2(x))))  (blocks.py:41)
        EBC_TRY(ebc::layernorm_fwd(dtype, s.X1, 0, 0, 0, p.ln2_g, p.ln2_b, s.H2, nullptr, s.m2, s.r2, M, TW, st));
        EBC_TRY(gemm(EBC_EPI_GELU, 0, s.H2, c.fc, s.G, p.b_fc, nullptr, s.A, M, TMLP, TW));
        EBC_TRY(gemm(EBC_EPI_RESID, 1, s.G, c.proj, lay.X[l + 1], p.b_proj, s.X1, nullptr, M, TW, TMLP));
    }
    // ln_final on the EOT rows, then the projection (text_encoder.py:50-52): B operand = text_projection^T [embed][512]
    EBC_TRY(ebc_prep_weights_1x1(dtype, w->text_projection, lay.tproj, lay.tproj_t, TW, embed, stream));
    hipLaunchKernelGGL(text_eot_gather_kernel, dim3((NB + 3) / 4), dim3(256), 0, st, lay.X[layers], eot, lay.Xe, NB, Lt);
    EBC_CHECK_LAUNCH();
    EBC_TRY(ebc::layernorm_fwd(dtype, lay.Xe, 0, 0, 0, w->ln_final_g, w->ln_final_b, lay.He, nullptr, lay.mf, lay.rf, NB, TW, st));
    EBC_TRY(gemm(EBC_EPI_STORE, 1, lay.He, lay.tproj_t, features, nullptr, nullptr, nullptr, NB, embed, TW));
    return EBC_OK;
}

extern "C" int ebc_text_backward(const EbcTextWeights* w, const EbcTextGrads* g, const int* ids, const int* eot,
                                 const int* uniq, const int* offs, const int* rows, int nu, int NB, int Lt, int dtype,
                                 void* ws, size_t wsb, const float* dfeatures, ebc_stream_t stream)
{
    EBC_TRY(text_weights_check(w, NB, Lt, dtype));
    if (!g || !g->layer || !g->token_embedding || !g->positional_embedding || !g->ln_final_g || !g->ln_final_b ||
        !g->text_projection || !ids || !eot || !uniq || !offs || !rows || !ws || !dfeatures)
        return EBC_E_ARG;
    if (nu < 1 || nu > NB * Lt) return EBC_E_ARG;
    const int layers = w->layers, embed = w->embed, M = NB * Lt;
    for (int l = 0; l < layers; ++l)
        if (!text_layer_ok(g->layer[l])) return EBC_E_ARG;
    const TLayout lay = text_carve(ws, NB, Lt, layers, embed, dtype, 1);
    if (lay.bytes > wsb) return EBC_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int Mp = lay.Mp;
    auto gemm = [&](int epi, int out_f32, const void* A, const void* Bm, void* C, const float* bias, const float* resid,
                    void* aux, int m, int n, int k) {
        return ebc::gemm_nt(dtype, epi, out_f32, A, Bm, C, bias, resid, aux, m, n, k, st);
    };
    // dW [R][C] f32 = dY^T [R][m] . Xin [m][C]: both operands transposed to K-contiguous rows of stride ld (pad columns zero)
    auto wgrad = [&](const void* dY, int R, const void* Xin, int C, void* tY, void* tX, float* dW, int m, int ld) -> int {
        EBC_TRY(ebc_transpose(dtype, dY, tY, m, R, ld, stream));
        EBC_TRY(ebc_transpose(dtype, Xin, tX, m, C, ld, stream));
        return ebc_gemm_wgrad(dtype, tY, tX, dW, R, C, ld, lay.wg, lay.wg_bytes, stream);
    };
    if (hipMemsetAsync(lay.zero0, 0, lay.zero_bytes, st) != hipSuccess) return EBC_E_LAUNCH;
    // features = He . proj: dHe = dF . proj^T, dproj = He^T . dF
    EBC_TRY(ebc::cast_f32(dtype, dfeatures, lay.dFt, (size_t)NB * embed, st));
    EBC_TRY(gemm(EBC_EPI_STORE, 0, lay.dFt, lay.tproj, lay.dHe, nullptr, nullptr, nullptr, NB, TW, embed));
    EBC_TRY(wgrad(lay.He, TW, lay.dFt, embed, lay.tE1, lay.tE2, g->text_projection, NB, 64));
    EBC_TRY(ebc::layernorm_bwd(dtype, 0, lay.dHe, lay.Xe, 0, 0, 0, lay.mf, lay.rf, w->ln_final_g, nullptr, lay.dXe, nullptr,
                               NB, TW, st));
    EBC_TRY(ebc_layernorm_param_grad(dtype, 0, lay.dHe, lay.Xe, lay.mf, lay.rf, g->ln_final_g, g->ln_final_b, NB, TW, stream));
    float *dX = lay.dXa, *dXn = lay.dXb;
    EBC_DTYPE_SWITCH(dtype, hipLaunchKernelGGL(text_eot_scatter_kernel<T>, dim3((M + 3) / 4), dim3(256), 0, st, lay.dXe, eot,
                                               dX, (T*)lay.dXt, NB, Lt));
    EBC_CHECK_LAUNCH();
    for (int l = layers - 1; l >= 0; --l) {
        const EbcTextLayer& p = w->layer[l];
        const EbcTextLayerGrads& d = g->layer[l];
        const TLayerW& c = lay.w[l];
        const TLayerSave& s = lay.s[l];
        // c_proj: dG' = (dX . W_proj) QuickGELU'(A); dW_proj = dX^T G; db_proj = column sums of dX
        EBC_TRY(gemm(EBC_EPI_GELU_BWD, 0, lay.dXt, c.proj_t, lay.dA, nullptr, nullptr, s.A, M, TMLP, TW));
        EBC_TRY(wgrad(lay.dXt, TW, s.G, TMLP, lay.tA, lay.tB, d.w_proj, M, Mp));
        EBC_TRY(ebc_colsum(dtype, 1, dX, d.b_proj, M, TW, stream));
        // c_fc
        EBC_TRY(gemm(EBC_EPI_STORE, 0, lay.dA, c.fc_t, lay.dH, nullptr, nullptr, nullptr, M, TW, TMLP));
        EBC_TRY(wgrad(lay.dA, TMLP, s.H2, TW, lay.tA, lay.tB, d.w_fc, M, Mp));
        EBC_TRY(ebc_colsum(dtype, 0, lay.dA, d.b_fc, M, TMLP, stream));
        // ln_2: dX1 = dX + LN'(dH)
        EBC_TRY(ebc::layernorm_bwd(dtype, 0, lay.dH, s.X1, 0, 0, 0, s.m2, s.r2, p.ln2_g, dX, dXn, lay.dXt, M, TW, st));
        EBC_TRY(ebc_layernorm_param_grad(dtype, 0, lay.dH, s.X1, s.m2, s.r2, d.ln2_g, d.ln2_b, M, TW, stream));
        std::swap(dX, dXn);
        // out_proj
        EBC_TRY(gemm(EBC_EPI_STORE, 0, lay.dXt, c.out_t, lay.dO, nullptr, nullptr, nullptr, M, TW, TW));
        EBC_TRY(wgrad(lay.dXt, TW, s.O, TW, lay.tA, lay.tB, d.w_out, M, Mp));
        EBC_TRY(ebc_colsum(dtype, 1, dX, d.b_out, M, TW, stream));
        // attention, in-projection
        EBC_TRY(ebc_attention_causal_bwd(dtype, s.QKV, lay.dO, s.O, s.lse, nullptr, lay.dQKV, NB, Lt, THEADS, stream));
        EBC_TRY(gemm(EBC_EPI_STORE, 0, lay.dQKV, c.qkv_t, lay.dH, nullptr, nullptr, nullptr, M, TW, TQKV));
        EBC_TRY(wgrad(lay.dQKV, TQKV, s.H1, TW, lay.tA, lay.tB, d.w_qkv, M, Mp));
        EBC_TRY(ebc_colsum(dtype, 0, lay.dQKV, d.b_qkv, M, TQKV, stream));
        // ln_1: dX_l = dX1 + LN'(dH)
        EBC_TRY(ebc::layernorm_bwd(dtype, 0, lay.dH, lay.X[l], 0, 0, 0, s.m1, s.r1, p.ln1_g, dX, dXn, lay.dXt, M, TW, st));
        EBC_TRY(ebc_layernorm_param_grad(dtype, 0, lay.dH, lay.X[l], s.m1, s.r1, d.ln1_g, d.ln1_b, M, TW, stream));
        std::swap(dX, dXn);
    }
    return ebc_text_embed_bwd(dX, uniq, offs, rows, nu, g->token_embedding, g->positional_embedding, NB, Lt, w->context, TW,
                              w->vocab, stream);
}
