// pixel.h -- pixel types and the arithmetic they are filtered in.
//
// The reference evaluates every scan in the pixel type P, with the float coefficients cast
// to P (lib/recfilter.cpp:324,335,338; lib/split.cpp:836,977,1107).  Floating pixels use
// their own type; integer pixels use unsigned 32-bit wrap-around arithmetic, which is the
// same ring the reference's int16/int32 expressions live in once the store truncates.
//
// The 16-bit floating-point pixel types (RF_F16, RF_BF16) deliberately depart from that "evaluate in the pixel
// type" rule: they are STORAGE types.  A sample is widened exactly to f32 when it is loaded, the coefficients, tails,
// carries, tables, pointwise stages and every intermediate are those of an RF_F32 plan, and the result is rounded once,
// to nearest even, at the final store:  out = round16(F_f32(widen(in))).  A recurrence evaluated in binary16 is
// useless, and the reference's apps have no 16-bit float case to be compatible with.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rf {

template <typename P> struct PixelTraits;

template <> struct PixelTraits<float> {
    using Acc = float;
    static __host__ __device__ inline Acc load(float v) { return v; }
    static __host__ __device__ inline float store(Acc v) { return v; }
    static inline Acc coef_from_double(double c) { return (float)c; }
    static constexpr bool is_integer = false;
};
template <> struct PixelTraits<double> {
    using Acc = double;
    static __host__ __device__ inline Acc load(double v) { return v; }
    static __host__ __device__ inline double store(Acc v) { return v; }
    static inline Acc coef_from_double(double c) { return c; }
    static constexpr bool is_integer = false;
};
template <> struct PixelTraits<int32_t> {
    using Acc = uint32_t;
    static __host__ __device__ inline Acc load(int32_t v) { return (uint32_t)v; }
    static __host__ __device__ inline int32_t store(Acc v) { return (int32_t)v; }
    static constexpr bool is_integer = true;
};
// (the conversions are the hardware's: v_cvt_f32_f16 / a shift on load, v_cvt_f16_f32 / v_cvt_pk_bf16_f32 on store --
// round to nearest even, overflow to +-inf, NaN propagates)
template <> struct PixelTraits<_Float16> {
    using Acc = float;
    static __host__ __device__ inline Acc load(_Float16 v) { return (float)v; }
    static __host__ __device__ inline _Float16 store(Acc v) { return (_Float16)v; }
    static inline Acc coef_from_double(double c) { return (float)c; }
    static constexpr bool is_integer = false;
};
template <> struct PixelTraits<__bf16> {
    using Acc = float;
    static __host__ __device__ inline Acc load(__bf16 v) { return (float)v; }
    static __host__ __device__ inline __bf16 store(Acc v) { return (__bf16)v; }
    static inline Acc coef_from_double(double c) { return (float)c; }
    static constexpr bool is_integer = false;
};
// Unsigned-byte planes on both sides (rf_pointwise_desc.in_dtype == RF_IO_U8) are a storage type in the same sense: the plan is
// the RF_F32 plan that reads the bytes (RF_IN_U8), and the f32 result is converted once, at the final store:
//     sat8(v) = (uint8) min(max(rint(v), 0), 255)      rint: to nearest, ties to even; below 0 -> 0, above 255 -> 255, NaN -> 0
// (fmaxf returns its other operand for a NaN).  Only the final-pass kernels of the fused path are instantiated with this
// destination type; no plan has it as its pixel type.
__host__ __device__ inline uint8_t sat8(float v) {
    return (uint8_t)(int32_t)__builtin_fminf(__builtin_fmaxf(__builtin_rintf(v), 0.0f), 255.0f);
}
template <> struct PixelTraits<uint8_t> {
    using Acc = float;
    static __host__ __device__ inline Acc load(uint8_t v) { return (float)v; }
    static __host__ __device__ inline uint8_t store(Acc v) { return sat8(v); }
    static inline Acc coef_from_double(double c) { return (float)c; }
    static constexpr bool is_integer = false;
};
template <> struct PixelTraits<int16_t> {
    using Acc = uint32_t;
    static __host__ __device__ inline Acc load(int16_t v) { return (uint32_t)(int32_t)v; }
    static __host__ __device__ inline int16_t store(Acc v) { return (int16_t)(uint16_t)v; }
    static constexpr bool is_integer = true;
};

// Two different questions the code used to ask with std::is_same<P, float>:
//   is_f32_arith<P>   the plan's arithmetic is f32 (neighbour-form carries, clamped sections, packed FMAs, pointwise stages):
//                     f32 pixels and the two 16-bit storage types
//   std::is_same<P, float>   the planes hold 4-byte floats (kernels that read the planes themselves as float: the LDS-DMA
//                     stream, the 3-D walk)
template <typename P> struct is_half_pixel { static constexpr bool value = false; };
template <> struct is_half_pixel<_Float16> { static constexpr bool value = true; };
template <> struct is_half_pixel<__bf16> { static constexpr bool value = true; };
template <typename P> struct is_f32_arith { static constexpr bool value = is_half_pixel<P>::value; };
template <> struct is_f32_arith<float> { static constexpr bool value = true; };

}  // namespace rf
