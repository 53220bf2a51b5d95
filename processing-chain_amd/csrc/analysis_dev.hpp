// Device side of the skeleton the analysis kernels share: a
// 256-lane workgroup of 4 waves owns a unit of a plane, the lanes' sums meet in
// a wave butterfly, the waves' in LDS in wave order, and one partial per unit
// goes to a finalize kernel: no atomics.
//   - the 16-B piece loader over bounds-checked buffer loads: metrics.hip,
//     framecrc.hip, stats.hip, align.hip, motion.hip;
//   - wave_sum: those and msssim.hip, vif.hip, adm.hip; block_sum and its two
//     halves block_gather, block_total: the last three and motion.hip;
//   - mirror_index, LevelPlane: vif.hip, adm.hip, motion.hip, msssim.hip.
// Host side: analysis_host.hpp.
#pragma once

#include <type_traits>

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

// Sums over the 256 lanes of a workgroup: x[i] goes through wave_sum, lane 0 of
// each wave puts it into s_red[wave][i], one barrier (block_gather), and the
// four are added in wave order as ((s0 + s1) + s2) + s3 (block_total).  That
// order is part of a double's bits: every kernel that promises run-to-run
// identical bits adds its waves here.  Every lane of the workgroup calls
// block_gather; any lane may then take block_total of value i (i may differ by
// lane).  block_sum is the two for every value, in every lane.  The caller
// keeps a barrier between these reads of s_red and its next writer.
template <typename V, int N>
__device__ __forceinline__ void block_gather(const V (&x)[N], V (*s_red)[N]) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const V v = wave_sum(x[i]);
        if (lane == 0) s_red[wave][i] = v;
    }
    __syncthreads();
}

template <typename V, int N>
__device__ __forceinline__ V block_total(const V (*s_red)[N], int i) {
    return ((s_red[0][i] + s_red[1][i]) + s_red[2][i]) + s_red[3][i];
}

template <typename V, int N>
__device__ __forceinline__ void block_sum(V (&x)[N], V (*s_red)[N]) {
    block_gather(x, s_red);
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = block_total(s_red, i);
}

// Index i of an axis of n samples under the mirrored border that does not
// repeat the edge sample (-i reads i, n - 1 + i reads n - 1 - i).  An index
// more than one reflection away (it only reaches positions that do not exist)
// is clamped, so every load goes to an element of the plane.
__device__ __forceinline__ int mirror_index(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// One plane of one level of a pyramid: the samples themselves (T) at scale 0,
// the context's workspace (uint32 sums or doubles) after that.
struct LevelPlane {
    const uint8_t *base;
    int64_t ls;
};

// Element (y, x) as a double: a sample brought to the 8-bit scale by mul (a
// power of two: exact), a double of the workspace as it is.
template <typename T>
__device__ __forceinline__ double level_sample(const LevelPlane &p, int y, int x, double mul) {
    const T v = reinterpret_cast<const T *>(p.base + (int64_t)y * p.ls)[x];
    if constexpr (std::is_same<T, double>::value) return v;
    else return (double)v * mul;
}

// Tap q of a symmetric window of n taps (g[q] and g[n - 1 - q] are the same
// bits) within its first half: reading that half alone halves the scalar
// registers a window takes.
__host__ __device__ constexpr int sym_tap(int q, int n) { return q < n - 1 - q ? q : n - 1 - q; }

// A pair of samples as the doubles an LDS row holds.
__device__ __forceinline__ double2 as_double2(double2 v) { return v; }
__device__ __forceinline__ double2 as_double2(uint2 v) { return make_double2((double)v.x, (double)v.y); }

// The windowed five moments of two planes (msssim_unit, vif_stat): the N x N
// window g x g over {a, b, a^2, b^2, a b} at COLS = 256 columns, one per lane,
// and nin - (N - 1) rows.  Per input row i of the band:
//   - fetch(i, halo, own, extra) gives the lane's (a, b) of column `lane` and,
//     where `halo` (lanes 0 .. N - 2), of column COLS + lane, as an S (uint2 or
//     double2) that is widened only when it goes into one of two LDS rows (one
//     barrier a row): the next row's loads are issued before this row is
//     worked on and are not waited for until then;
//   - H: the lane reads its N neighbours from LDS and filters the five
//     quantities into slot i % N of a ring of N rows x 5 doubles held in
//     registers (the row loop is unrolled by N, so every slot is a fixed
//     register);
//   - V: from row N - 1 on, the ring's N rows give the five weighted sums of
//     the window whose last row this is, and pos(v) takes them.
// Tap 0 is a product, every later one an fma, in tap order: the order is part
// of the result's bits.  `busy` (wave-uniform): some lane of the wave has a
// column that counts; the others only move rows.  The caller keeps a barrier
// between this and the next writer of s_row.
template <int N, int COLS, typename S, typename Fetch, typename Pos>
__device__ __forceinline__ void window_moments(double2 (*s_row)[COLS + N - 1], const double *g, int nin, bool busy,
                                               Fetch fetch, Pos pos) {
    const int tid = threadIdx.x;
    const bool halo = tid < N - 1;
    S nx, nh{};  // the next row's samples
    fetch(0, halo, nx, nh);
    double ring[N][5];
    for (int i0 = 0; i0 < nin; i0 += N) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const int i = i0 + j;  // input row of the band; its ring slot is j
            if (i >= nin) break;   // uniform
            double2 *row = s_row[i & 1];
            row[tid] = as_double2(nx);
            if (halo) row[COLS + tid] = as_double2(nh);
            // this row has landed; the row before it has been read by every wave, so the
            // next one may overwrite it
            __syncthreads();
            if (i + 1 < nin) fetch(i + 1, halo, nx, nh);  // travels while this row is filtered
            if (!busy) continue;
            double h[5];
#pragma unroll
            for (int q = 0; q < N; ++q) {
                const double2 v = row[tid + q];
                const double m[5] = {v.x, v.y, v.x * v.x, v.y * v.y, v.x * v.y};
#pragma unroll
                for (int c = 0; c < 5; ++c) h[c] = q ? __builtin_fma(g[sym_tap(q, N)], m[c], h[c]) : g[0] * m[c];
            }
#pragma unroll
            for (int c = 0; c < 5; ++c) ring[j][c] = h[c];
            if (i < N - 1) continue;  // uniform
            double v[5];
#pragma unroll
            for (int q = 0; q < N; ++q)  // tap q is input row i - (N - 1) + q
#pragma unroll
                for (int c = 0; c < 5; ++c) {
                    const double x = ring[(j + 1 + q) % N][c];
                    v[c] = q ? __builtin_fma(g[sym_tap(q, N)], x, v[c]) : g[0] * x;
                }
            pos(v);
        }
    }
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
