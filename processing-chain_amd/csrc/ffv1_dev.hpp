// What the FFV1 encoder (ffv1.hip) and decoder (ffv1dec.hip) share on the
// device, each written once: slice geometry, prediction and the threshold
// quantiser, the table blob, the context-state layout with its HOT / COLD
// split, and the register-block helpers of the two range coders.
#pragma once
#include <cstring>

#include "device.hpp"

namespace pp {

// ---- slice geometry (RFC 9043 4.6: slice_x .. in units of the grid) ---------
// the first sample of part i when n samples are cut into `parts`
__device__ __host__ inline int slice_edge(int i, int n, int parts) { return (int)((int64_t)i * n / parts); }

struct SliceGeo {
    int frame, s, sx, sy, x0, x1, y0, y1, lw, lh, cw, ch;
    __device__ __host__ int len() const { return lw * lh + 2 * cw * ch; }
};
__device__ __host__ inline SliceGeo slice_geo(int g, int w, int h, int nh, int nv, int hsub, int vsub) {
    SliceGeo q;
    const int per = nh * nv;
    q.frame = g / per;
    q.s = g - q.frame * per;
    q.sy = q.s / nh;
    q.sx = q.s - q.sy * nh;
    q.x0 = slice_edge(q.sx, w, nh);
    q.x1 = slice_edge(q.sx + 1, w, nh);
    q.y0 = slice_edge(q.sy, h, nv);
    q.y1 = slice_edge(q.sy + 1, h, nv);
    q.lw = q.x1 - q.x0;
    q.lh = q.y1 - q.y0;
    q.cw = (q.lw + (1 << hsub) - 1) >> hsub;
    q.ch = (q.lh + (1 << vsub) - 1) >> vsub;
    return q;
}

// ---- prediction and quantiser ------------------------------------------------
__device__ __forceinline__ int median3(int a, int b, int c) { return max(min(a, b), min(max(a, b), c)); }

// ffv1_quant (ffv1host.cpp) as ALU code: the number of thresholds <= |d|,
// odd-mirrored (unused thresholds are 1024)
__device__ __forceinline__ int dquant(int d, const int (&thr)[5]) {  // d already & 0xFF
    const int m = d < 128 ? d : (d == 128 ? 127 : 256 - d);
    const int q = (m >= thr[0]) + (m >= thr[1]) + (m >= thr[2]) + (m >= thr[3]) + (m >= thr[4]);
    return d < 128 ? q : -q;
}

// ---- table blob ----------------------------------------------------------------
// zero[256] | one[256] | crc[256] u32 | x^(8 * 2^j) mod P [32] u32.  The
// encoder's blob ends after the CRC table; the decoder's wave-parallel CRC
// check needs the powers as well.
constexpr int kTabZero = 0;                  // next state after a 0 decision
constexpr int kTabOne = 256;                 // after a 1 decision
constexpr int kTabStates = 512;              // bytes of zero | one, the coders' LDS copy
constexpr int kTabCrc = kTabStates;          // CRC-32 byte table (crc_table)
constexpr int kTabXp = kTabCrc + 256 * 4;    // powers of x for the CRC of split messages
constexpr int kTabBytes = kTabXp;            // blob without the powers
constexpr int kTabBytesXp = kTabXp + 32 * 4; // with them

// ---- context states ------------------------------------------------------------
// A context's 32 state bytes are split in two 16-byte halves.  HOT, the block
// a coder holds in 4 VGPRs and loads on every context switch: [0] zero flag,
// [1..5] exponent bits 0..4, [6..10] sign for e = 0..4, [11..14] mantissa
// bits 0..3 -- every state a residual below 32 in magnitude touches.  COLD,
// read and written in place only once an exponent reaches 5: [0..4] exponent
// bits 5..9, [5..9] sign for e = 5..9, [10..14] mantissa bits 4..8.  (FFmpeg's
// states 21 and 31 serve > 10-bit samples only; byte 15 of a half is unused.)
inline void split_states(const uint8_t *st, uint8_t hot[16], uint8_t cold[16]) {
    std::memset(hot, 128, 16);
    std::memset(cold, 128, 16);
    hot[0] = st[0];
    for (int i = 0; i < 5; ++i) {
        hot[1 + i] = st[1 + i];
        hot[6 + i] = st[11 + i];
        cold[i] = st[6 + i];
        cold[5 + i] = st[16 + i];
        cold[10 + i] = st[26 + i];
    }
    for (int i = 0; i < 4; ++i) hot[11 + i] = st[22 + i];
}

// The halves of 64 neighbouring slots (slices, or the decoder's chains) are
// interleaved: context k of slot s at [s / 64][k][s % 64][16], so one 128-B
// line holds a context's half of 8 neighbours -- a context that is hot in one
// slice is hot in the slices beside it.  `slot_bytes` is what one slot takes
// in a group (the encoder keeps a group's cold halves behind its hot ones:
// both halves; the decoder keeps them in an array of their own: one).  From
// a slot's context 0 the next context is kCtxStride further.
constexpr int kCtxStride = 64 * 16;
template <typename P>  // P: const uint8_t or uint8_t
__device__ __forceinline__ P *state_at(P *base, int slot, int ctx, int64_t slot_bytes) {
    P *const c = base + (int64_t)(slot >> 6) * (64 * slot_bytes) + (int64_t)ctx * kCtxStride;
    // (the lane as an index of 16-byte elements: as a byte offset the `& 63`
    // is folded into the shift before inlining, and the kernels can no
    // longer share it with their other per-lane addresses)
    return (P *)((const uint4 *)c + (slot & 63));
}

// state byte k of a block held in N dwords (k a compile-time constant after
// unrolling: no dynamic register indexing)
template <int N>
__device__ __forceinline__ uint32_t st_get(const uint32_t (&b)[N], int k) { return (b[k >> 2] >> ((k & 3) * 8)) & 0xFFu; }
template <int N>
__device__ __forceinline__ void st_put(uint32_t (&b)[N], int k, uint32_t v) {
    b[k >> 2] = (b[k >> 2] & ~(0xFFu << ((k & 3) * 8))) | (v << ((k & 3) * 8));
}

// one 16-byte half between memory and 4 VGPRs
__device__ __forceinline__ void hblk_load(uint32_t (&b)[4], const uint8_t *p) {
    const uint4 x = *reinterpret_cast<const uint4 *>(p);
    b[0] = x.x; b[1] = x.y; b[2] = x.z; b[3] = x.w;
}
__device__ __forceinline__ void hblk_store(uint8_t *p, const uint32_t (&b)[4]) {
    *reinterpret_cast<uint4 *>(p) = make_uint4(b[0], b[1], b[2], b[3]);
}

}  // namespace pp
