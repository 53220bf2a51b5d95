// Device-side pieces shared by the scaler kernels (scale.hip: general
// scale_kernel, strip_u16.hip / strip_u8.hip: strip_kernel instances): plane
// jobs and launch arguments (scale_plan.hpp, shared with the host planner),
// ordered-dither matrix, 16-B buffer loads, v_dot2 helpers and LDS staging
// stores.  See scale.hip for the reference semantics.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "common.hpp"
#include "device.hpp"
#include "scale_plan.hpp"

namespace pp {

static __constant__ uint8_t c_dither[8][8] = {
    {36, 68, 60, 92, 34, 66, 58, 90},  {100, 4, 124, 28, 98, 2, 122, 26},
    {52, 84, 44, 76, 50, 82, 42, 74},  {116, 20, 108, 12, 114, 18, 106, 10},
    {32, 64, 56, 88, 38, 70, 62, 94},  {96, 0, 120, 24, 102, 6, 126, 30},
    {48, 80, 40, 72, 54, 86, 46, 78},  {112, 16, 104, 8, 118, 22, 110, 14},
};

// the same matrix, one row per 64-bit word (byte k = column k): a wave-uniform
// row index makes it one scalar load, the lane's 4 columns one rotate
constexpr uint64_t dither_row64(const uint8_t (&r)[8]) {
    uint64_t v = 0;
    for (int k = 7; k >= 0; --k) v = (v << 8) | r[k];
    return v;
}
constexpr uint8_t kDither[8][8] = {
    {36, 68, 60, 92, 34, 66, 58, 90},  {100, 4, 124, 28, 98, 2, 122, 26},
    {52, 84, 44, 76, 50, 82, 42, 74},  {116, 20, 108, 12, 114, 18, 106, 10},
    {32, 64, 56, 88, 38, 70, 62, 94},  {96, 0, 120, 24, 102, 6, 126, 30},
    {48, 80, 40, 72, 54, 86, 46, 78},  {112, 16, 104, 8, 118, 22, 110, 14},
};
static __constant__ uint64_t c_dither64[8] = {
    dither_row64(kDither[0]), dither_row64(kDither[1]), dither_row64(kDither[2]), dither_row64(kDither[3]),
    dither_row64(kDither[4]), dither_row64(kDither[5]), dither_row64(kDither[6]), dither_row64(kDither[7]),
};

// Register prefetch of up to kPF 16-byte source chunks per lane (software
// pipelining of the staging: issued before the vertical pass of the previous
// chunk, committed to LDS after it).
constexpr int kPF = 4;

template <typename ST>
struct Prefetch {
    uint4 v[kPF];
};

// Unaligned-source fallback: element loads, zero past the plane edge.
template <typename ST>
__device__ inline uint4 load16_scalar(const ST *g, int col, int sw) {
    constexpr int CH = 16 / sizeof(ST);
    uint4 r = {0, 0, 0, 0};
    ST tmp[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) tmp[e] = (col + e < sw) ? g[col + e] : ST(0);
    __builtin_memcpy(&r, tmp, 16);
    return r;
}

// Bounds-checked 16-B load through the frame plane's buffer resource: bytes at
// or past num_records read as 0 without touching memory, so lanes with no
// chunk (and the right edge of the plane's last row) need no branch.  Samples
// past a row's end inside the plane come from the next row; the compacted
// filters give them zero weight.
#ifndef PP_SRC_LOAD_AUX
#define PP_SRC_LOAD_AUX 0
#endif
__device__ inline uint4 bload16(__amdgpu_buffer_rsrc_t rs, int off) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, PP_SRC_LOAD_AUX);
    uint4 r;
    __builtin_memcpy(&r, &v, 16);
    return r;
}

typedef int16_t v2i16 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// a.lo*b.lo + a.hi*b.hi + c in the VOP3P form (the compiler's v_dot2c form
// needs the accumulator copied into the destination first)
__device__ inline int dot2_acc(v2i16 a, v2i16 b, int c) {
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// c + a.lo*b.lo + a.hi*b.hi with b a wave-uniform SGPR and the accumulator c
// a separate VGPR (VOP3P form): the compiler's v_dot2c form would first copy c
// into the destination, one v_mov per output
__device__ inline int dot2_sv(v2i16 a, int32_t b_s, int c) {
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "s"(b_s), "v"(a), "v"(c));
    return r;
}

// a.lo*b.lo + a.hi*b.hi with a zero accumulator as an inline constant (the
// compiler otherwise zeroes a register for the v_dot2c form)
__device__ inline int dot2_first(v2i16 a, v2i16 b) {
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// 16-bit sources are stored as s ^ 0x8000 (= s - 32768 as int16) so any u16
// sample is an exact signed operand of v_dot2_i32_i16; the H pass adds the
// 32768 * sum(coef) bias back.  8-bit samples are stored as-is (<= 255).
template <typename ST>
__device__ inline void store16(uint16_t *lds_dst, uint4 v) {
    if constexpr (sizeof(ST) == 2) {
        v.x ^= 0x80008000u; v.y ^= 0x80008000u; v.z ^= 0x80008000u; v.w ^= 0x80008000u;
        *reinterpret_cast<uint4 *>(lds_dst) = v;
    } else {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint4 lo, hi;
        lo.x = __builtin_amdgcn_perm(0, w[0], 0x0c010c00u);
        lo.y = __builtin_amdgcn_perm(0, w[0], 0x0c030c02u);
        lo.z = __builtin_amdgcn_perm(0, w[1], 0x0c010c00u);
        lo.w = __builtin_amdgcn_perm(0, w[1], 0x0c030c02u);
        hi.x = __builtin_amdgcn_perm(0, w[2], 0x0c010c00u);
        hi.y = __builtin_amdgcn_perm(0, w[2], 0x0c030c02u);
        hi.z = __builtin_amdgcn_perm(0, w[3], 0x0c010c00u);
        hi.w = __builtin_amdgcn_perm(0, w[3], 0x0c030c02u);
        reinterpret_cast<uint4 *>(lds_dst)[0] = lo;
        reinterpret_cast<uint4 *>(lds_dst)[1] = hi;
    }
}

// ---------------------------------------------------------------------------
// strip_kernel: the common-case scaler (every plane in 256-column strips,
// 16-B aligned source rows, <= 8 vertical tap pairs, <= 10-bit samples).
//
// Same strip/segment/chunk walk and LDS layout as scale_kernel, but every
// loop is wave-uniform (wave = row group, lane = 4 adjacent columns), so the
// control flow is scalar branches instead of exec-mask bookkeeping:
//   H pass: one lane computes 4 adjacent output columns of a row PAIR.  The 4
//     windows share one 8-B aligned base in the staged row (hbase4), read as
//     HW dwords with ds_read_b64 (one read serves all 4 outputs); per output
//     the taps are re-laid over those dwords (hcoefw, zero outside its
//     window), so each output is HW v_dot2_i32_i16 with no realignment, and
//     the 8 results go to the window as one ds_write_b128.
//   V pass: a wave owns an output row; its tap pairs come from a padded
//     [dh][8] table through scalar loads (SGPR operands of v_dot2), the
//     window rows through ds_read_b128 (4 columns x 2 rows), one 8-B store.
//   Kept row pairs are read before the chunk's first barrier and written
//     after it, so the move costs no extra barrier.
// The next chunk's source rows are prefetched into registers right after the
// first barrier, so their HBM latency overlaps both passes.
#define kconst __attribute__((address_space(4)))  // constant address space: uniform loads become s_load
template <typename T>
__device__ inline const kconst T *as_kconst(const void *p) {
    return (const kconst T *)(uintptr_t)p;
}
constexpr int kKeepRegs = 2;  // kept pairs per wave carried in registers (4 waves -> 8 pairs)
constexpr int kStripThreads = kThreads;

template <typename ST>
__device__ inline void store_raw16(uint16_t *lds_dst, uint4 v) {
    if constexpr (sizeof(ST) == 2) {
        *reinterpret_cast<uint4 *>(lds_dst) = v;  // <= 10-bit samples are exact int16 operands
    } else {
        store16<ST>(lds_dst, v);                  // 8-bit: widen to 16-bit
    }
}


using KernelFn = void (*)(const ScaleArgs);
// strip_kernel instances (strip_u16.hip, strip_u8.hip): OUTB 8/10, HW window
// dwords, VTM = largest V tap-pair count over the planes; nullptr if not built
// tw: strip width (= threads) 256 or 512
KernelFn pick_strip_u16(int outb, int hw, int vtm, int tw);
KernelFn pick_strip_u8(int outb, int hw, int vtm, int tw);
// chain plans: first stage to 8 bit, second stage into `out2` (8/10) bits
KernelFn pick_strip_chain_u16(int out2, int hw, int vtm);
KernelFn pick_strip_chain_u8(int out2, int hw, int vtm);
KernelFn pick_strip_luma_u16(int hw, int vtm);  // FUSE 9: a chain's luma launch into 10 bits
KernelFn pick_strip_luma_u8(int hw, int vtm);
KernelFn pick_strip_chroma_u16(int hw, int vtm);  // FUSE 11: a chain's chroma launch into 10 bits
KernelFn pick_strip_chroma_u8(int hw, int vtm);
// GENERIC_UYVY plans: 8-bit samples stored straight into the packed uyvy422 row
KernelFn pick_strip_packed_u16(int hw, int vtm);
KernelFn pick_strip_packed_u8(int hw, int vtm);
int strip_vtm_bucket(int vtp);
// strip.hpp's strip_clamp_path() as a function of the instance's parameters
// (SB source sample bytes; OUTB the kernel's first-stage output bits), so the
// host can report it (pp_scale_plan_instances)
constexpr bool strip_clamp_rule(int sb, int outb, int hw, int vtm, int fuse) {
    return !(fuse >= 8 && hw >= 10) && !(sb == 1 && outb == 8 && hw == 4 && (fuse >= 8 || vtm >= 5));
}

}  // namespace pp
