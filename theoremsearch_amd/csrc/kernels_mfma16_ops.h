// Matrix primitives of the 16x16 MFMA shapes on gfx950, shared by the search kernel (kernels_mfma16.h), the int8 screen
// (kernels_screen8_tile.h, kernels_screen8.h), the rank kernel (kernels_rank_mfma.h), the encoder's attention
// (kernels_attention.h) and the threshold sample (kernels_sample.h): the fragment types, the MFMA statements with pinned
// register classes, the placed LDS read, the scalar-based LDS-DMA piece, the ring's landing wait and the accumulators' wait states.
#pragma once
#include "kernels_mfma.h"

namespace ts {

typedef __attribute__((ext_vector_type(4))) float f32x4;
// a corpus fragment in flight (one ds_read_b128): four dwords, so that copies of it are four plain register moves
typedef __attribute__((ext_vector_type(4))) unsigned frag16;

// MFMA statements with pinned register classes: accumulator and corpus fragment in VGPRs, query fragment in a VGPR
// ("v" forms) or an AGPR ("a" forms) quadruple.  No pads inside: the A fragment comes from a ds_read behind the k-step's
// explicit lgkmcnt wait (lds_read16 below), the query fragments are written once before the loop, accumulators chain
// MFMA -> MFMA; the only non-MFMA reader of an accumulator is the epilogue, behind mfma16_settle().
__device__ __forceinline__ void mfma16_v_first(f32x4& acc, const frag16& a, const bf16x8& b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma16_v(f32x4& acc, const frag16& a, const bf16x8& b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma16_a_first(f32x4& acc, const frag16& a, const bf16x8& b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "a"(b));
}
__device__ __forceinline__ void mfma16_a(f32x4& acc, const frag16& a, const bf16x8& b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "a"(b));
}
// int8 screen (I8): v_mfma_i32_16x16x64_i8, 64 bytes of K per 16-byte operand; the accumulator registers hold i32 bits
__device__ __forceinline__ void mfma8_v_first(f32x4& acc, const frag16& a, const bf16x8& b) {
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma8_v(f32x4& acc, const frag16& a, const bf16x8& b) {
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma8_a_first(f32x4& acc, const frag16& a, const bf16x8& b) {
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "a"(b));
}
__device__ __forceinline__ void mfma8_a(f32x4& acc, const frag16& a, const bf16x8& b) {
    asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "a"(b));
}
// fp32 rows (F32): v_mfma_f32_16x16x4_f32, one float of the corpus chunk x one float of the query chunk per instruction
__device__ __forceinline__ void mfma16f_v_first(f32x4& acc, float a, float b) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma16f_v(f32x4& acc, float a, float b) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma16f_a(f32x4& acc, float a, float b) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "a"(b));
}
__device__ __forceinline__ void mfma16f_a_first(f32x4& acc, float a, float b) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "a"(b));
}
// A-fragment read with a fixed place in the instruction stream (asm volatile statements keep their order among themselves):
// the compiler does not know the result is asynchronous - every consumer sits behind an explicit s_waitcnt lgkmcnt below.
template <int OFF>
__device__ __forceinline__ void lds_read16(frag16& dst, unsigned addr) {
    static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}
// LDS-DMA piece with a wave-uniform base in SGPRs, a 32-bit per-lane offset and an immediate: no vector arithmetic per
// piece.  The immediate is added to the global AND to the LDS address (LDS address = M0 + immediate + 16 * lane), so the
// caller passes lds_dst - IMM.
#ifndef TS16_DMA_IMM_LDS
#define TS16_DMA_IMM_LDS 1
#endif
template <int IMM, bool NT = true>
__device__ __forceinline__ void lds_dma16s(unsigned voff, const void* sbase, unsigned lds_dst) {
    static_assert(IMM >= 0 && IMM < 4096, "13-bit signed immediate");
    if constexpr (NT)
        asm volatile(
            "s_mov_b32 m0, %2\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %0, %1 offset:%3" TS_DMA_POLICY
            :
            : "v"(voff), "s"(sbase), "s"(lds_dst), "n"(IMM)
            : "memory");
    else
        asm volatile(
            "s_mov_b32 m0, %2\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %0, %1 offset:%3"
            :
            : "v"(voff), "s"(sbase), "s"(lds_dst), "n"(IMM)
            : "memory");
}
// The same piece as two statements with an MFMA between them (the late-test screen's steady tiles): M0 = lds_dst + OFF a gap
// ahead - the MFMA is the wait state the write of M0 needs in front of the load, and the sum needs no register of its own - then
// the load alone.  Nothing the compiler makes between the two may write M0 (tests/test_screen8_gaps_isa_cpu.py reads the ISA).
template <int OFF>
__device__ __forceinline__ void lds_dma16s_m0(unsigned lds_dst) {
    if constexpr (OFF == 0) asm volatile("s_mov_b32 m0, %0" : : "s"(lds_dst));
    else asm volatile("s_add_i32 m0, %0, %1" : : "s"(lds_dst), "n"(OFF) : "scc");
}
template <int IMM, bool NT = true>
__device__ __forceinline__ void lds_dma16s_go(unsigned voff, const void* sbase) {
    static_assert(IMM >= 0 && IMM < 4096, "13-bit signed immediate");
    if constexpr (NT) asm volatile("global_load_lds_dwordx4 %0, %1 offset:%2" TS_DMA_POLICY : : "v"(voff), "s"(sbase), "n"(IMM) : "memory");
    else asm volatile("global_load_lds_dwordx4 %0, %1 offset:%2" : : "v"(voff), "s"(sbase), "n"(IMM) : "memory");
}
// Every outstanding fragment read has landed; names the whole ring, so that no copy of a ring register the compiler may
// need where control flow merges (end of a tile, steady / general branch) is placed above it.
template <int N>
__device__ __forceinline__ void lds_ring_landed(frag16 (&af)[N]) {
    static_assert(N == 6 || N == 8, "ring of 3 or 4 k-steps, two row blocks");
    if constexpr (N == 6)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(af[0]), "+v"(af[1]), "+v"(af[2]), "+v"(af[3]), "+v"(af[4]), "+v"(af[5]));
    else
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(af[0]), "+v"(af[1]), "+v"(af[2]), "+v"(af[3]), "+v"(af[4]), "+v"(af[5]),
                     "+v"(af[6]), "+v"(af[7]));
}
// wait states between the last MFMA writing an accumulator and its first VALU reader (hipcc pads nothing for asm)
template <int NB>
__device__ __forceinline__ void mfma16_settle(f32x4 (&acc)[2][NB]) {
    if constexpr (NB == 4)
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[0][3]), "+v"(acc[1][0]),
                     "+v"(acc[1][1]), "+v"(acc[1][2]), "+v"(acc[1][3]));
    else if constexpr (NB == 3)
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[1][0]), "+v"(acc[1][1]),
                     "+v"(acc[1][2]));
    else if constexpr (NB == 2)
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[1][0]), "+v"(acc[1][1]));
    else
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0][0]), "+v"(acc[1][0]));
}

}  // namespace ts
