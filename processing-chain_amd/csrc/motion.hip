// VMAF-style motion of a luma sequence (spec PP-MOTION-1) on gfx950:
// for every shown frame the sum of absolute differences between its blurred
// luma plane and the blurred plane of the frame shown before it.  The blur is
// the separable five-tap integer filter {3571, 16004, 26386, 16004, 3571} / 65536,
// columns first, a rounding after each pass, borders mirrored without repeating
// the edge sample.  motion and motion2 are host arithmetic (pixpath/motion.py).
// The taps, roundings and scale are libvmaf's integer motion as recalled; parity
// with libvmaf is unpinned: no libvmaf exists to compare with.
//
// Layout: a workgroup (256 lanes, 4 waves) owns one unit = (segment of kMoSeg
// consecutive shown frames, tile of kMoTileRows rows x 62 pieces) and walks
// the segment's frames over its tile, as siti_kernel and stat_kernel walk
// theirs.  Wave v owns rows v*16 .. v*16+15 of the tile, a lane one 16-B piece
// (16 or 8 samples) of every row: bounds-checked buffer loads through
// analysis_dev.hpp, element-wise off the 16-B grid with the same results.
// Lanes 0 and 63 of a wave are the tile's column halo: they load and filter
// like the others and own no output, so a tile has 62 * 16 / es output columns
// and starts one piece left of them (the halo columns are recomputed per tile).
//
// Per frame a wave streams its 16 + 4 input rows (mirrored row indices)
// through a ring of five raw pieces held in registers; the row loop is
// unrolled, so every slot is a fixed register.  From the fifth row on:
//   V:  t = (sum f[k] x[k] + 2^(d-1)) >> d for the lane's samples; the lane
//       puts them as 16-bit values into its wave's LDS row;
//   mirror: four lanes copy t(1), t(2), t(w-2), t(w-3) into the slots of
//       columns -1, -2, w, w+1 where the row holds them;
//   H:  the lane reads its samples and two to either side back from LDS and
//       gives B = (sum f[k] t[k] + 32768) >> 16, packs two to a dword, clears
//       what lies outside the plane, adds |B - B_prev| (v_sad_u16) and keeps
//       B as B_prev for the next frame: 16 rows x 8 (4) dwords in registers.
// No blurred sample ever goes to memory; a source frame is read once per
// (tile, segment) plus the halo.  The first frame of a segment (the frame shown
// before it, or `prev`) is blurred only to seed B_prev.
//
// Exactness (all arithmetic 32-bit unsigned, no float):
//   x:    min(stored, 2^d - 1) <= 1023 (255)
//   V:    accumulator <= 65536 * 1023 + 512 < 2^27; t <= 65472 (65280 at 8 bits)
//   H:    accumulator <= 65536 * 65472 + 32768 < 2^32; B <= 65472: 16 bits
//   sad:  per lane and frame <= 16 rows * 16 samples * 65472 < 2^24; wave
//         (butterfly, 32 bits) < 2^30; tile, frame in 64 bits: a plane of
//         < 2^31 samples gives < 2^47
// Pitch padding of a ragged last piece is loaded as it is and filtered, but
// reaches no output: the slots of columns w and w + 1 are overwritten by the
// mirror and everything right of them is cleared from B.
// Reduction: block_sum (four waves < 2^30 each: 32 bits) -> one 64-bit partial
// per (frame, tile); motion_finalize adds a frame's
// partials in tile order.  No atomics: two runs give the same bits.
#include <algorithm>

#include "analysis_dev.hpp"
#include "analysis_host.hpp"

namespace pp {

constexpr int kMoWaves = 4;                         // waves per workgroup
constexpr int kMoLaneRows = 16;                     // rows of a tile one wave owns
constexpr int kMoTileRows = kMoWaves * kMoLaneRows; // rows of a tile
constexpr int kMoPieces = 62;                       // output pieces of a tile's row (64 lanes less the halo)
constexpr int kMoSeg = 4;                           // shown frames a workgroup walks
constexpr uint32_t kMoF0 = 3571, kMoF1 = 16004, kMoF2 = 26386;

struct MoArgs {
    const uint8_t *src, *prev;  // prev: the frame shown before frame 0 of the launch (any valid frame if none)
    int64_t ls, fs, pls;
    int w, h, rb;               // samples and bytes of a row; rows
    int tx, tiles;              // tiles across; tiles of a plane
    int nk;                     // shown frames of this launch
    int first_absent;           // frame 0 of the launch has no previous frame
    uint64_t *part;             // [nk][tiles]
    uint64_t *sad;              // [nk]
    int32_t idx[kFrameMap];     // source frame of shown frame k
};

// One workgroup per (segment, tile) of the launch, segment-major.
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(256) void motion_kernel(const MoArgs a) {
    constexpr int ES = sizeof(T), SPP = 16 / ES, NP = SPP / 2;  // samples, 16-bit pairs of a piece
    constexpr int D = ES == 2 ? 10 : 8;
    constexpr int ROWD = 64 * NP + 2;  // dwords of an LDS row: a pair of slots either side of the wave's samples
    __shared__ __align__(16) uint32_t s_t[kMoWaves][ROWD];
    __shared__ uint32_t s_red[kMoWaves][1];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int seg = blockIdx.x / a.tiles, tile = blockIdx.x - seg * a.tiles;
    const int band = tile / a.tx, tcol = tile - band * a.tx;
    const int w = a.w, h = a.h, rb = a.rb;
    const int xt0 = tcol * kMoPieces * SPP - SPP;  // column of the wave's first sample (the left halo lane's)
    const int x0 = xt0 + lane * SPP;               // column of the lane's first sample
    const int c = x0 * ES;                         // its byte
    const bool in = c >= 0 && c < rb;              // the piece has a byte inside the row
    const int cl = in ? c : 0;                     // the element-wise loader clamps from the right only
    const int r0 = band * kMoTileRows + wave * kMoLaneRows;  // the wave's first output row
    // samples of the lane's piece that are outputs: none in the halo lanes
    const int nv = (lane >= 1 && lane <= kMoPieces) ? min(max(w - x0, 0), SPP) : 0;
    // the mirror's four copies, one lane each: slot of column x is x - xt0 + 2
    int mdst = -1, msrc = 0;
    {
        const int dcol = lane == 0 ? -1 : lane == 1 ? -2 : lane == 2 ? w : w + 1;
        const int scol = lane == 0 ? 1 : lane == 1 ? 2 : lane == 2 ? w - 2 : w - 3;
        const int d = dcol - xt0, s = scol - xt0;
        if (lane < 4 && d >= 0 && d < 64 * SPP && s >= 0 && s < 64 * SPP) { mdst = d + 2; msrc = s + 2; }
    }
    uint16_t *const row16 = reinterpret_cast<uint16_t *>(s_t[wave]);
    uint32_t *const row32 = s_t[wave];

    uint32_t pv[kMoLaneRows][NP];  // B_prev of the lane's samples, two to a dword
#pragma unroll
    for (int u = 0; u < kMoLaneRows; ++u)
#pragma unroll
        for (int d = 0; d < NP; ++d) pv[u][d] = 0;

    const int k0 = seg * kMoSeg, k1 = min(a.nk, k0 + kMoSeg);
    for (int k = k0 - 1; k < k1; ++k) {  // k0 - 1: the frame shown before the segment seeds B_prev
        const bool seed = k < k0;
        const bool outer = k < 0;  // the launch's prev, with a pitch of its own
        const uint8_t *base = outer ? a.prev : a.src + (int64_t)a.idx[max(k, 0)] * a.fs;
        const int64_t ls = outer ? a.pls : a.ls;
        const auto rs = plane_rsrc<ALIGNED>(base, h, ls, rb);
        // frame-invariant values: recomputed per frame instead of held as scalar masks and
        // one row offset per ring row
        int nvf = nv, r0f = r0;
        asm volatile("" : "+v"(nvf));
        asm volatile("" : "+v"(r0f));
        r0f = __builtin_amdgcn_readfirstlane(r0f);
        uint32_t ring[5][4];
        uint32_t nxt[4];
        load_piece<T, ALIGNED>(nxt, rs, base, ls, mirror_index(r0f - 2, h), h, cl, rb, in);
        uint32_t sad = 0;
#pragma unroll
        for (int i = 0; i < kMoLaneRows + 4; ++i) {  // input row r0 - 2 + i of the band, ring slot i % 5
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t q = nxt[d];
                if constexpr (ES == 2) {  // x = min(stored, 1023), both halves
                    const uint32_t lo = min(q & 0xffffu, 1023u), hi = min(q >> 16, 1023u);
                    q = lo | (hi << 16);
                }
                ring[i % 5][d] = q;
            }
            if (i + 1 < kMoLaneRows + 4)  // travels while this row is filtered
                load_piece<T, ALIGNED>(nxt, rs, base, ls, mirror_index(r0f - 2 + i + 1, h), h, cl, rb, in);
            if (i < 4) continue;
            const int u = i - 4;  // output row r0 + u: taps are ring slots (i - 4 .. i) % 5
            // V
            uint32_t t[SPP];
#pragma unroll
            for (int j = 0; j < SPP; ++j) {
                uint32_t x[5];
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    const uint32_t dw = ring[(u + q) % 5][j * ES / 4];
                    if constexpr (ES == 2) x[q] = (j & 1) ? dw >> 16 : dw & 0xffffu;
                    else x[q] = (dw >> (8 * (j & 3))) & 0xffu;
                }
                t[j] = (kMoF0 * (x[0] + x[4]) + kMoF1 * (x[1] + x[3]) + kMoF2 * x[2] + (1u << (D - 1))) >> D;
            }
#pragma unroll
            for (int d = 0; d < NP; ++d) row32[1 + lane * NP + d] = t[2 * d] | (t[2 * d + 1] << 16);
            __syncthreads();  // the wave's row has landed
            if (mdst >= 0) row16[mdst] = row16[msrc];
            __syncthreads();  // and its mirrored slots
            uint32_t e[NP + 2];
#pragma unroll
            for (int d = 0; d < NP + 2; ++d) e[d] = row32[lane * NP + d];
            // a row belongs to one wave, whose LDS accesses keep their order: the next row's
            // stores stay behind these loads
            if (r0f + u >= h) continue;  // wave-uniform: the row lies below the plane
            // H: tt[j] is column x0 - 2 + j
            uint32_t tt[SPP + 4];
#pragma unroll
            for (int j = 0; j < SPP + 4; ++j) tt[j] = (j & 1) ? e[j >> 1] >> 16 : e[j >> 1] & 0xffffu;
#pragma unroll
            for (int d = 0; d < NP; ++d) {
                uint32_t b[2];
#pragma unroll
                for (int o = 0; o < 2; ++o) {
                    const int j = 2 * d + o;
                    b[o] = (kMoF0 * (tt[j] + tt[j + 4]) + kMoF1 * (tt[j + 1] + tt[j + 3]) + kMoF2 * tt[j + 2] + 32768u) >> 16;
                }
                const int n = nvf - 2 * d;  // samples of this pair that are outputs
                const uint32_t cur = (b[0] | (b[1] << 16)) & (n >= 2 ? 0xffffffffu : n == 1 ? 0xffffu : 0u);
                sad = __builtin_amdgcn_sad_u16(cur, pv[u][d], sad);
                pv[u][d] = cur;
            }
        }
        if (seed) continue;  // uniform
        // 32 bits hold the four waves: 64 rows x 62 x 16 columns x 65472 = 4.16e9 < 2^32 = 4.29e9
        // (kMoTileRows x kMoPieces x 16 / es samples of at most 65472; 8 bits is the larger case)
        static_assert((uint64_t)kMoTileRows * kMoPieces * 16 * 65472 < (uint64_t)1 << 32, "a tile's sum needs 64 bits");
        uint32_t tot[1] = {sad};
        block_sum(tot, s_red);  // the next write of s_red lies behind the next frame's row barriers
        if (threadIdx.x == 0) a.part[(int64_t)k * a.tiles + tile] = tot[0];
    }
}

// One lane per shown frame of the launch: its partials in tile order;
// UINT64_MAX for a frame without a previous one and for planes under 3 x 3.
__global__ __launch_bounds__(64) void motion_finalize(const uint64_t *part, int nk, int tiles, int first_absent,
                                                      int all_absent, uint64_t *sad) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= nk) return;
    uint64_t s = ~uint64_t(0);
    if (!all_absent && !(k == 0 && first_absent)) {
        s = 0;
        for (int t = 0; t < tiles; ++t) s += part[(int64_t)k * tiles + t];
    }
    sad[k] = s;
}

}  // namespace pp

using namespace pp;

extern "C" int pp_motion(pp_ctx *ctx, int bitdepth, int w, int h, const void *src, int64_t src_linesize,
                         int64_t src_frame_stride, int nsrc, const int32_t *index, int n, const void *prev,
                         int64_t prev_linesize, uint64_t *sad, void *stream) {
    if (!ctx || !src || !sad) PP_FAIL(PP_ERR_INVALID, "null argument");
    LumaPlanes lp;
    const LumaClip pool{src, src_linesize, src_frame_stride, nsrc}, before{prev, prev_linesize, 0, 1};
    if (int e = luma_checks(lp, bitdepth, w, h, pool, before, true, index, n, kIndexMap)) return e;
    const int es = lp.es;
    if (n == 0) return PP_OK;

    hipStream_t st = static_cast<hipStream_t>(stream);
    PP_HIP(hipSetDevice(ctx->device));
    const bool none = w < 3 || h < 3;  // one reflection does not suffice: every entry absent
    MoArgs a{};
    a.src = static_cast<const uint8_t *>(src);
    a.ls = src_linesize; a.fs = src_frame_stride;
    a.w = w; a.h = h; a.rb = (int)lp.g.rb;
    const int cols = kMoPieces * 16 / es;  // output columns of a tile
    a.tx = (w + cols - 1) / cols;
    a.tiles = a.tx * ((h + kMoTileRows - 1) / kMoTileRows);
    const int per = frames_per_launch(n);
    if (!none) {
        if (int e = grow(ctx->mot, sizeof(uint64_t) * (size_t)per * a.tiles)) return e;
        a.part = static_cast<uint64_t *>(ctx->mot.buf);
    }
    const auto kern = es == 2 ? PP_PICK(motion_kernel, uint16_t, lp.aligned) : PP_PICK(motion_kernel, uint8_t, lp.aligned);
    each_launch(n, per, [&](int k0, int nk) {
        MoArgs b = a;
        b.nk = nk;
        fill_map(b.idx, index, k0, nk);
        b.first_absent = put_shown_before(b, index, k0, prev, prev_linesize);
        b.sad = sad + k0;
        if (!none) {
            const int segs = (b.nk + kMoSeg - 1) / kMoSeg;
            // a workgroup per (segment, tile): far below 2^31 for planes inside the 2 GiB range and kFrameMap frames
            hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)segs * a.tiles)), dim3(256), 0, st, b);
        }
        hipLaunchKernelGGL(motion_finalize, dim3((b.nk + 63) / 64), dim3(64), 0, st, b.part, b.nk, a.tiles,
                           b.first_absent, none ? 1 : 0, b.sad);
    });
    PP_HIP(hipGetLastError());
    return PP_OK;
}
