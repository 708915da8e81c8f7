// Element helpers of the storage-typed kernels (pool.hip, grouping.hip, train.hip, bn_train.hip, pool_train.hip): a 16-bit element travels as an
// unsigned short, arithmetic is fp32, T = __bf16 or _Float16 selects the encoding; fp32 storage is E = T = float.
#pragma once
#include "gv_common.h"

namespace gvlp_elem {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ float up(unsigned short b) { return (float)__builtin_bit_cast(T, b); }
template <typename T>
__device__ __forceinline__ float up(float v) { return v; }      // fp32 storage (T = float): the identity
template <typename T>
__device__ __forceinline__ auto down(float v) {
    if constexpr (sizeof(T) == 4) {
        return v;
    } else {
        const T h = (T)v;
        return __builtin_bit_cast(unsigned short, h);
    }
}

template <typename T>
__device__ __forceinline__ void unpack8(u32x4 v, float (&f)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f[2 * j] = up<T>((unsigned short)(v[j] & 0xffffu));
        f[2 * j + 1] = up<T>((unsigned short)(v[j] >> 16));
    }
}
template <typename T>
__device__ __forceinline__ u32x4 pack8(const float (&f)[8]) {
    u32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (unsigned)down<T>(f[2 * j]) | ((unsigned)down<T>(f[2 * j + 1]) << 16);
    return v;
}

// load / store VEC (8 or 1) consecutive elements as fp32
template <typename T, int VEC>
__device__ __forceinline__ void load_v(const unsigned short* p, float (&f)[8]) {
    if constexpr (VEC == 8) unpack8<T>(*reinterpret_cast<const u32x4*>(p), f);
    else f[0] = up<T>(*p);
}
template <typename T, int VEC>
__device__ __forceinline__ void store_v(unsigned short* p, const float (&f)[8]) {
    if constexpr (VEC == 8) *reinterpret_cast<u32x4*>(p) = pack8<T>(f);
    else *p = down<T>(f[0]);
}

// one 16-byte quad of storage elements <-> fp32 registers: 8 elements of a 16-bit type T, or 4 floats (E = float)
template <typename E, typename T>
__device__ __forceinline__ void unpackq(u32x4 v, float (&f)[8]) {
    if constexpr (sizeof(E) == 2) {
        unpack8<T>(v, f);
    } else {
        const f32x4 w = __builtin_bit_cast(f32x4, v);
        f[0] = w[0]; f[1] = w[1]; f[2] = w[2]; f[3] = w[3];
    }
}
template <typename E, typename T>
__device__ __forceinline__ u32x4 packq(const float (&f)[8]) {
    if constexpr (sizeof(E) == 2) {
        return pack8<T>(f);
    } else {
        const f32x4 w = {f[0], f[1], f[2], f[3]};
        return __builtin_bit_cast(u32x4, w);
    }
}

// the same access pattern on fp32 storage (VEC = 4: one 16-byte load), so kernels templated on the pointer type serve
// both storages
template <typename T, int VEC>
__device__ __forceinline__ void load_v(const float* p, float (&f)[8]) {
    if constexpr (VEC == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
    } else {
        f[0] = *p;
    }
}
template <typename T, int VEC>
__device__ __forceinline__ void store_v(float* p, const float (&f)[8]) {
    if constexpr (VEC == 4) {
        f32x4 v = {f[0], f[1], f[2], f[3]};
        *reinterpret_cast<f32x4*>(p) = v;
    } else {
        *p = f[0];
    }
}

// Pixel accessor of the forward kernels (pool.hip, grouping.hip) and the training pools (pool_train.hip): the NN channels
// from channel ch of pixel pix of a tensor with pixel stride ld elements, as fp32 registers.  NN = 1 is the scalar access;
// a vector access (4 or 8 fp32, 8 of a 16-bit type) moves whole 16-byte quads, which the host checks for.  at() advances
// the base by whole pixels.  The three-plane accessor P3Px is in conv_x3_epi.h.
template <typename E, typename T, int NN>
struct Px {
    using elem = E;
    static constexpr int N = NN;
    static constexpr int PER = 16 / sizeof(E);                   // elements of a quad
    // the tensor from pixel pix on: a kernel that walks a row takes the row's address once
    template <typename P>
    static __device__ __forceinline__ P at(P base, size_t pix, int ld) { return base + pix * (size_t)ld; }
    static __device__ __forceinline__ void load(const E* base, size_t pix, int ld, int ch, float (&f)[NN]) {
        const E* p = base + pix * (size_t)ld + ch;
        if constexpr (NN == 1) {
            f[0] = up<T>(*p);
        } else {
#pragma unroll
            for (int q = 0; q < NN / PER; ++q) {
                float w[8];
                unpackq<E, T>(*reinterpret_cast<const u32x4*>(p + q * PER), w);
#pragma unroll
                for (int e = 0; e < PER; ++e) f[q * PER + e] = w[e];
            }
        }
    }
    static __device__ __forceinline__ void store(E* base, size_t pix, int ld, int ch, const float (&f)[NN]) {
        E* p = base + pix * (size_t)ld + ch;
        if constexpr (NN == 1) {
            *p = down<T>(f[0]);
        } else {
#pragma unroll
            for (int q = 0; q < NN / PER; ++q) {
                float w[8];
#pragma unroll
                for (int e = 0; e < PER; ++e) w[e] = f[q * PER + e];
                *reinterpret_cast<u32x4*>(p + q * PER) = packq<E, T>(w);
            }
        }
    }
};

}  // namespace gvlp_elem
