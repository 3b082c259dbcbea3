// bf16 / MFMA device primitives shared by every translation unit of libsei_hip.so (gfx950), included from sei_common.h:
// one definition of the vector types, of the float <-> bf16 conversions that the bf16 parity tests rest on, of the
// MFMA wrappers and of the counted waits, instead of a private copy per file.
#pragma once

using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using v4s = __attribute__((ext_vector_type(4))) short;
using v8s = __attribute__((ext_vector_type(8))) short;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

// float -> bf16 bits, round to nearest even (the hardware conversion), and back (exact)
__device__ __forceinline__ unsigned short sei_f2bf(float v) {
    const __bf16 b = (__bf16)v;
    return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float sei_bf2f(unsigned short v) { return __uint_as_float((unsigned)v << 16); }
// two floats -> a bf16 pair in one 32-bit word, `a` in the low half
__device__ __forceinline__ unsigned sei_pack2_bf16(float a, float b) {
    return (unsigned)sei_f2bf(a) | ((unsigned)sei_f2bf(b) << 16);
}

// D = A B + C on the matrix cores, bf16 operands (8 per lane), float32 accumulators
__device__ __forceinline__ f32x16 sei_mfma32(bf16x8 a, bf16x8 b, f32x16 c) {      // 32 x 32 x 16
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 sei_mfma16(bf16x8 a, bf16x8 b, f32x4 c) {        // 16 x 16 x 32
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// counted wait: at most N vector-memory operations (loads, stores and LDS-DMA pieces alike, in issue order) still in flight
template <int N>
__device__ __forceinline__ void sei_wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is six bits");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// LDS writes of this wave done, then the barrier (a bare s_barrier does not wait for them; __syncthreads would also
// wait for every global load and LDS-DMA piece in flight)
__device__ __forceinline__ void sei_lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}
