// Device side of the skeleton the analysis reducers share (metrics.hip,
// framecrc.hip, stats.hip): a 256-lane workgroup of 4 waves owns a
// unit of a plane, a lane takes 16-B pieces of rows through bounds-checked
// buffer loads, the lanes' sums meet in a wave butterfly, and one partial per
// unit goes to a finalize kernel: no atomics.  Host side: analysis_host.hpp.
#pragma once

#include "device.hpp"

namespace pp {

// The plane a tile lies in; tile0[p] is the first tile of plane p of a frame.
__device__ inline int plane_of_tile(const int *tile0, int tile) {
    return tile >= tile0[2] ? 2 : tile >= tile0[1] ? 1 : 0;
}

// Sum over the 64 lanes of a wave, in every lane: the xor butterfly over the
// offsets 1, 2, 4 .. 32 in that order (the order is part of a double's result).
template <typename V>
__device__ __forceinline__ V wave_sum(V x) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// Descriptor of one frame's plane of ph rows of rb bytes at pitch ls, for
// load_piece.  A load straddling num_records reads 0 as a whole, so the last
// row counts up to its 16-B-rounded extent wb.  ALIGNED means ls is a multiple
// of 16 and ls >= rb, hence ls >= wb: the range ends inside the last row's
// pitch and needs no min(ls, wb).  Not ALIGNED: no range, load_piece clamps.
template <bool ALIGNED>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const uint8_t *base, int ph, int64_t ls, int64_t rb) {
    const int64_t wb = (rb + 15) & ~int64_t(15);
    return uniform_rsrc(base, ALIGNED ? (int)((int64_t)(ph - 1) * ls + wb) : 0);
}

// The 16-B piece at byte c of row `row` as four dwords, zero outside the plane.
// `in`: the caller's test that the piece has a byte inside the plane; the other
// lanes go to kOobOff (no memory access).  ALIGNED: one buffer load; a row >= ph
// of an `in` lane lies past the descriptor's range and reads 0 too, provided
// row * ls + c < 2^32 (the entry point's range check).  Pitch padding between
// rb and the piece's end comes back as it is: mask_piece.  Otherwise (pointers
// or pitches off the 16-B grid) element by element of type T, padding as 0.
template <typename T, bool ALIGNED>
__device__ __forceinline__ void load_piece(uint32_t q[4], __amdgpu_buffer_rsrc_t rs, const uint8_t *base, int64_t ls,
                                           int row, int ph, int c, int rb, bool in) {
    if constexpr (ALIGNED) {
        const uint32_t voff = in ? (uint32_t)row * (uint32_t)ls + (uint32_t)c : (uint32_t)kOobOff;
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0);
        __builtin_memcpy(q, &v, 16);
    } else {
        constexpr int EPD = 4 / sizeof(T);  // elements per dword
        // every load goes to an element of the plane (clamped); the select drops the others
        const T *r = reinterpret_cast<const T *>(base + (int64_t)min(row, ph - 1) * ls);
        const int x0 = c / (int)sizeof(T), n = rb / (int)sizeof(T);
        const bool ok = in && row < ph;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t v = 0;
#pragma unroll
            for (int e = 0; e < EPD; ++e) {
                const int x = x0 + d * EPD + e;
                const uint32_t s = r[min(x, n - 1)];
                v |= ((ok && x < n) ? s : 0u) << (8 * sizeof(T) * e);
            }
            q[d] = v;
        }
    }
}

// Clears the bytes of a piece past the first nb (nb <= 0: all, >= 16: none):
// the ragged edge of a row whose extent is no multiple of 16 B.
__device__ __forceinline__ void mask_piece(uint32_t q[4], int nb) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int n = nb - 4 * d;  // bytes of this dword inside the row
        q[d] &= n >= 4 ? 0xffffffffu : n <= 0 ? 0u : (1u << (8 * n)) - 1u;
    }
}

}  // namespace pp
