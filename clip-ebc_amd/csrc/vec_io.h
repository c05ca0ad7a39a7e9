// Typed vector loads and stores of 4 and 8 consecutive elements (float, _Float16, __bf16), f32 on the register side:
// 8 / 16 B for the 16-bit types, 16 / 32 B for f32.  p is aligned to the access.
#pragma once
#include <hip/hip_runtime.h>

namespace ebc {

template <class T> __device__ __forceinline__ float4 ld4(const T* p) {
    typedef T t4 __attribute__((ext_vector_type(4)));
    const t4 v = *reinterpret_cast<const t4*>(p);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
template <> __device__ __forceinline__ float4 ld4<float>(const float* p) { return *reinterpret_cast<const float4*>(p); }
// ... <-> float[4]
template <class T> __device__ __forceinline__ void ld4(const T* p, float* v) {
    const float4 x = ld4<T>(p);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
}
template <class T> __device__ __forceinline__ void st4(T* p, const float* v) {
    typedef T t4 __attribute__((ext_vector_type(4)));
    *reinterpret_cast<t4*>(p) = t4{(T)v[0], (T)v[1], (T)v[2], (T)v[3]};
}
template <class T> __device__ __forceinline__ void st4(T* p, float4 v) {
    const float a[4] = {v.x, v.y, v.z, v.w};
    st4<T>(p, a);
}
template <> __device__ __forceinline__ void st4<float>(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// 8 consecutive elements <-> float[8] (16 B for the 16-bit types, 32 B for f32)
template <class T> __device__ __forceinline__ void ld8(const T* p, float* v) {
    typedef T t8 __attribute__((ext_vector_type(8)));
    const t8 x = *reinterpret_cast<const t8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)x[i];
}
template <class T> __device__ __forceinline__ void st8(T* p, const float* v) {
    typedef T t8 __attribute__((ext_vector_type(8)));
    t8 x;
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = (T)v[i];
    *reinterpret_cast<t8*>(p) = x;
}

}  // namespace ebc
