// Luma SSE of every distorted frame against a band of reference frames (spec
// PP-ALIGN-1) on gfx950: the sums a temporal alignment searches.
//   sse[k][c] = sum (dist[k] - ref[first[k] + c])^2 over the w x h samples,
// UINT64_MAX where first[k] + c names no reference frame.
//
// Layout: a tile is kAlnTileRows (64) rows x kAlnTileBytes (1024 B) of the
// luma plane.  A workgroup (256 lanes, 4 waves) owns one unit = (distorted
// frame k, tile).  Wave v holds rows v*16 .. v*16+15 of the tile, a lane one
// 16-B piece of each of them (kAlnLaneRows pieces, one column): the
// distorted tile is loaded ONCE into 64 VGPRs and stays there while the
// workgroup walks the ncand candidates, loading the same pieces of reference
// frame first[k] + c, kAlnGroup of them in flight per lane.  So the distorted
// bytes are read once per call and the reference bytes ncand times; the grid
// is tile-major with the XCD-aware numbering (xcd_remap), so the workgroups
// resident on one XCD hold the same few tiles of neighbouring k and walk the
// same reference frames at about the same time: of the batch's reads of a
// reference tile one goes to HBM, the others meet in that XCD's L2 (or in the
// Infinity Cache for another XCD).
// Loads are the analysis kernels' (analysis_dev.hpp): bounds-checked 16-B
// buffer loads, rows below the plane and columns right of the row read 0 in
// BOTH inputs and add nothing; the bytes of a ragged last piece that lie in
// the pitch padding are masked in both (RAGGED).  A source off the 16-B grid
// (pointer, linesize or frame stride) is read element by element with explicit
// clamps instead (ALIGNED = false).  That path is taken for BOTH inputs when
// either is off the grid, and it reads the distorted row anew per candidate
// from the caches: a tile held in registers needs the fully unrolled row loop,
// and unrolled the element loads spill.  Equal results in all four
// combinations of aligned and unaligned dist and ref.
//
// Arithmetic, per lane and candidate (64 dwords = 16 pieces):
//   8 bit:  sum (a-b)^2 = sum a^2 + sum b^2 - 2 sum a b with v_dot4_u32_u8 on
//           the dwords as they are; sum a^2 is formed once per tile.
//   16 bit: D = |a - b| per 16-bit half (v_pk_max/min/sub_u16), split into its
//           bytes H and L (d = 256 H + L), three v_dot2_u32_u16 sums:
//           sum d^2 = 65536 sum H^2 + 512 sum H L + sum L^2.
// Exactness (every stored value, nothing masked):
//   8 bit:  a dword's dot <= 4 * 255^2 < 2^18; lane (64 dwords) sum a^2,
//           sum b^2, sum a b each < 2^24, the lane's SSE < 2^24: 32 bits;
//           wave (butterfly) < 2^30: 32 bits; tile and frame in 64 bits
//   16 bit: a dword's dot of bytes <= 2 * 255^2 < 2^17; lane sums H^2, H L,
//           L^2 each < 2^23: 32 bits; the lane's SSE = 65536 HH + 512 HL + LL
//           < 2^39 and everything after it in 64 bits: wave < 2^45, tile
//           < 2^47, frame < 2^31 samples (the buffer range) * 2^32 = 2^63
// so no sum wraps and UINT64_MAX is never a sum.  Reduction: lane -> wave (xor
// butterfly) -> workgroup (4 values through LDS, kAlnChunk candidates per
// exchange) -> one partial per (unit, candidate); align_finalize adds a
// (frame, candidate)'s partials in tile order.  Integers, no atomics: the
// result does not depend on any order.
#include <algorithm>
#include <type_traits>

#include "analysis_dev.hpp"
#include "analysis_host.hpp"

namespace pp {

constexpr int kAlnLaneBytes = 16;  // one load per lane and piece
constexpr int kAlnLanes = 64;      // a wave's span of a row
constexpr int kAlnWaves = 4;       // waves per workgroup
constexpr int kAlnLaneRows = 16;   // rows of a tile one wave holds: pieces per lane
constexpr int kAlnTileRows = kAlnWaves * kAlnLaneRows;
constexpr int kAlnTileBytes = kAlnLanes * kAlnLaneBytes;
constexpr int kAlnGroup = 4;       // reference pieces (loads) in flight per lane
constexpr int kAlnChunk = 32;      // candidates between two exchanges through LDS

struct AlnArgs {
    const uint8_t *dist, *ref;
    int64_t dls, dfs, rls, rfs;
    int rb, ph;      // bytes of a row that count; rows
    int tx, tiles;   // tiles across a row; tiles of a frame
    int nk;          // distorted frames of this launch
    int nref, ncand;
    uint64_t *part;  // [nk][tiles][ncand]
    uint64_t *sse;   // [nk][ncand]
    int32_t first[kFrameMap];
};

typedef uint16_t aln_v2u16 __attribute__((ext_vector_type(2)));

template <int ES, bool ALIGNED, bool RAGGED>
__device__ __forceinline__ void align_unit(const AlnArgs &a, int k, int tile, uint64_t (*s_part)[kAlnWaves]) {
    using T = std::conditional_t<ES == 2, uint16_t, uint8_t>;
    using Acc = std::conditional_t<ES == 2, uint64_t, uint32_t>;  // a lane's and a wave's SSE
    const int band = tile / a.tx, tx = tile - band * a.tx;
    const int rb = a.rb, ph = a.ph;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = tx * kAlnTileBytes + lane * kAlnLaneBytes;   // byte column of the lane's pieces
    const int r0 = band * kAlnTileRows + wave * kAlnLaneRows;  // the wave's first row
    const int nrows = min(max(ph - r0, 0), kAlnLaneRows);      // and how many it has (wave-uniform)
    const int nb = min(max(rb - c, 0), kAlnLaneBytes);         // bytes of a piece inside the row
    uint32_t mask[4] = {~0u, ~0u, ~0u, ~0u};                   // RAGGED: those bytes
    mask_piece(mask, nb);
    const uint8_t *db = a.dist + (int64_t)k * a.dfs;
    const auto drs = plane_rsrc<ALIGNED>(db, ph, a.dls, rb);

    // ALIGNED: the distorted tile, once
    uint32_t dv[kAlnLaneRows][4];
    uint32_t saa = 0;  // 8 bit: sum a^2 of the lane
    if constexpr (ALIGNED) {
#pragma unroll
        for (int u = 0; u < kAlnLaneRows; ++u) {
            load_piece<T, true>(dv[u], drs, db, a.dls, r0 + u, ph, c, rb, r0 + u < ph && nb > 0);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                if constexpr (RAGGED) dv[u][d] &= mask[d];
                if constexpr (ES == 1) saa = __builtin_amdgcn_udot4(dv[u][d], dv[u][d], saa, false);
            }
        }
    }

    const int64_t f0 = a.first[k];
    uint64_t *out = a.part + ((int64_t)k * a.tiles + tile) * a.ncand;
    for (int c0 = 0; c0 < a.ncand; c0 += kAlnChunk) {
        const int c1 = min(a.ncand, c0 + kAlnChunk);
        for (int cc = c0; cc < c1; ++cc) {
            const int64_t j = f0 + cc;
            if (j < 0 || j >= a.nref) continue;  // absent (uniform): align_finalize writes UINT64_MAX
            const uint8_t *rbase = a.ref + j * a.rfs;
            const auto rrs = plane_rsrc<ALIGNED>(rbase, ph, a.rls, rb);
            uint32_t s0 = 0, s1 = 0, s2 = 0;  // 8 bit: sum b^2, sum a b; 16 bit: sums H^2, H L, L^2
            // one dword of each input
            auto add = [&](uint32_t va, uint32_t vb) {
                if constexpr (ES == 1) {
                    s0 = __builtin_amdgcn_udot4(vb, vb, s0, false);
                    s1 = __builtin_amdgcn_udot4(va, vb, s1, false);
                } else {
                    const aln_v2u16 x = __builtin_bit_cast(aln_v2u16, va), y = __builtin_bit_cast(aln_v2u16, vb);
                    const aln_v2u16 dd = __builtin_elementwise_max(x, y) - __builtin_elementwise_min(x, y);
                    const uint32_t D = __builtin_bit_cast(uint32_t, dd);
                    const aln_v2u16 H = __builtin_bit_cast(aln_v2u16, (D >> 8) & 0x00ff00ffu);
                    const aln_v2u16 L = __builtin_bit_cast(aln_v2u16, D & 0x00ff00ffu);
                    s0 = __builtin_amdgcn_udot2(H, H, s0, false);
                    s1 = __builtin_amdgcn_udot2(H, L, s1, false);
                    s2 = __builtin_amdgcn_udot2(L, L, s2, false);
                }
            };
            if constexpr (ALIGNED) {
#pragma unroll
                for (int g = 0; g < kAlnLaneRows; g += kAlnGroup) {
                    if (g >= nrows) break;  // the rows below the plane are 0 in both inputs
                    uint32_t q[kAlnGroup][4];
#pragma unroll
                    for (int u = 0; u < kAlnGroup; ++u)
                        load_piece<T, true>(q[u], rrs, rbase, a.rls, r0 + g + u, ph, c, rb, r0 + g + u < ph && nb > 0);
#pragma unroll
                    for (int u = 0; u < kAlnGroup; ++u)
#pragma unroll
                        for (int d = 0; d < 4; ++d) add(dv[g + u][d], RAGGED ? q[u][d] & mask[d] : q[u][d]);
                }
            } else {
                // element by element, a row at a time and both inputs anew (the loop stays
                // rolled: a register-resident tile cannot be indexed by a rolled loop)
                saa = 0;
#pragma unroll 1
                for (int u = 0; u < nrows; ++u) {
                    uint32_t qa[4], qb[4];
                    load_piece<T, false>(qa, drs, db, a.dls, r0 + u, ph, c, rb, nb > 0);
                    load_piece<T, false>(qb, rrs, rbase, a.rls, r0 + u, ph, c, rb, nb > 0);
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        if constexpr (ES == 1) saa = __builtin_amdgcn_udot4(qa[d], qa[d], saa, false);
                        add(qa[d], qb[d]);
                    }
                }
            }
            Acc s;
            if constexpr (ES == 1) s = saa + s0 - 2 * s1;
            else s = ((uint64_t)s0 << 16) + ((uint64_t)s1 << 9) + s2;
            s = wave_sum(s);
            if (lane == 0) s_part[cc - c0][wave] = s;
        }
        __syncthreads();  // the chunk's wave sums have landed
        const int t = threadIdx.x;
        if (t < c1 - c0) {
            const int64_t j = f0 + c0 + t;
            if (j >= 0 && j < a.nref) out[c0 + t] = s_part[t][0] + s_part[t][1] + s_part[t][2] + s_part[t][3];
        }
        __syncthreads();  // and have been read: the next chunk may overwrite them
    }
}

// 1-D grid over the (tile, frame) units, tile-major, with the XCD-aware
// numbering: an XCD holds a contiguous range of units, that is a few tiles of
// every frame of the launch, whose candidates are the same reference tiles.
template <int ES, bool ALIGNED, bool RAGGED>
__global__ __launch_bounds__(256) void align_kernel(const AlnArgs a) {
    __shared__ uint64_t s_part[kAlnChunk][kAlnWaves];
    const int64_t total = (int64_t)a.nk * a.tiles;
    for (int64_t u = xcd_remap(blockIdx.x, gridDim.x); u < total; u += gridDim.x) {
        const int tile = (int)(u / a.nk);
        align_unit<ES, ALIGNED, RAGGED>(a, (int)(u - (int64_t)tile * a.nk), tile, s_part);
    }
}

// One lane per (frame, candidate): its partials in tile order, or UINT64_MAX.
__global__ __launch_bounds__(256) void align_finalize(const AlnArgs a) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= (int64_t)a.nk * a.ncand) return;
    const int k = (int)(o / a.ncand), c = (int)(o - (int64_t)k * a.ncand);
    const int64_t j = (int64_t)a.first[k] + c;
    uint64_t s = ~uint64_t(0);
    if (j >= 0 && j < a.nref) {
        const uint64_t *q = a.part + (int64_t)k * a.tiles * a.ncand + c;
        s = 0;
        for (int t = 0; t < a.tiles; ++t) s += q[(int64_t)t * a.ncand];
    }
    a.sse[o] = s;
}

}  // namespace pp

using namespace pp;

extern "C" int pp_frame_sse_band(pp_ctx *ctx, int bitdepth, int w, int h, const void *dist, int64_t dist_linesize,
                                 int64_t dist_frame_stride, int ndist, const void *ref, int64_t ref_linesize,
                                 int64_t ref_frame_stride, int nref, const int32_t *first, int ncand, uint64_t *sse,
                                 void *stream) {
    if (!ctx || !dist || !ref || !first || !sse) PP_FAIL(PP_ERR_INVALID, "null argument");
    LumaPlanes lp;
    if (int e = luma_open(lp, bitdepth, w, h)) return e;
    if (ndist < 0) PP_FAIL(PP_ERR_INVALID, "ndist %d < 0", ndist);
    if (nref < 0) PP_FAIL(PP_ERR_INVALID, "nref %d < 0", nref);
    if (ncand < 1) PP_FAIL(PP_ERR_INVALID, "ncand %d < 1", ncand);
    // a tile's rows below the plane stay inside the buffer range too
    if (int e = luma_plane(lp, dist, dist_linesize, dist_frame_stride, "dist ", kAlnTileRows)) return e;
    if (int e = luma_plane(lp, ref, ref_linesize, ref_frame_stride, "ref ", kAlnTileRows)) return e;
    if (int e = luma_close(lp)) return e;
    const int es = lp.es;
    const PlaneGeom &g = lp.g;
    if (ndist == 0) return PP_OK;

    AlnArgs a{};
    put_luma_pair(a, {ref, ref_linesize, ref_frame_stride, nref}, {dist, dist_linesize, dist_frame_stride, ndist});
    a.rb = (int)g.rb; a.ph = h;
    a.tx = (int)((g.rb + kAlnTileBytes - 1) / kAlnTileBytes);
    a.tiles = a.tx * ((h + kAlnTileRows - 1) / kAlnTileRows);
    a.nref = nref; a.ncand = ncand;
    const bool ragged = (g.rb & 15) != 0;

    hipStream_t st = static_cast<hipStream_t>(stream);
    PP_HIP(hipSetDevice(ctx->device));
    const int per = frames_per_launch(ndist);
    if (int e = grow(ctx->aln, sizeof(uint64_t) * (size_t)per * a.tiles * ncand)) return e;
    a.part = static_cast<uint64_t *>(ctx->aln.buf);

    const bool aligned = lp.aligned;  // one source off the 16-B grid: both go element by element
    const auto kern = es == 2 ? PP_PICK_EDGE(align_kernel, 2, aligned, ragged) : PP_PICK_EDGE(align_kernel, 1, aligned, ragged);
    // `first` travels in the kernel arguments as a frame map does
    each_launch(ndist, per, [&](int k0, int nk) {
        AlnArgs b = a;
        b.nk = nk;
        fill_map(b.first, first, k0, nk);
        b.dist += (int64_t)k0 * a.dfs;
        b.sse = sse + (int64_t)k0 * ncand;
        const int64_t units = (int64_t)b.nk * a.tiles;
        const int groups = (int)std::min<int64_t>(units, (int64_t)std::max(1, ctx->cus) * 8);
        hipLaunchKernelGGL(kern, dim3(groups), dim3(256), 0, st, b);
        const int64_t outs = (int64_t)b.nk * ncand;
        hipLaunchKernelGGL(align_finalize, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, b);
    });
    PP_HIP(hipGetLastError());
    return PP_OK;
}
