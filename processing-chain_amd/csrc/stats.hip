// Per-frame signal statistics of a frame batch (spec PP-STATS-1) on
// gfx950: for every frame and plane the histogram of the samples, the number
// of 10-bit samples at or above 1024 (`over`) and the sum of absolute
// differences to the previous frame (`sad`).  Everything the host reports
// (pixpath/stats.py) is arithmetic on these three exact integer arrays.
//
// Layout: a tile is kStTileRows (64) rows x kStTileBytes (1024 B) of one
// plane.  A workgroup (256 lanes, 4 waves) owns one unit = (chunk of
// kStFrames consecutive frames, tile) and walks the chunk's frames over its
// tile.  Wave v holds rows v*16 .. v*16+15 of the tile, a lane one 16-B piece
// of each of them (kStLaneRows pieces, one column), so a wave's load of one
// row is 1024 contiguous bytes.  The previous frame's 16 pieces stay in
// registers (64 VGPRs): with `sad` every sample is still read from HBM once,
// plus the frame before the chunk (1 / kStFrames more).  Loads are
// bounds-checked 16-B buffer loads, kStGroup in flight per lane; rows below
// the plane and columns right of the row read 0 without traffic, and the bytes
// of a ragged last piece that lie in the pitch padding are masked (RAGGED).
// Pointers, linesizes or frame strides off the 16-B grid: the same kernel with
// byte loads and explicit clamps (ALIGNED = false), equal results.  The piece
// loader, its mask, the descriptor and the butterfly: analysis_dev.hpp.
//
// Histogram: per workgroup an LDS sub-histogram of one (frame, tile), bin-major
// with R copies of every bin (hist[bin * R + lane % R], R = 8 for 1024 bins,
// 16 for 256 bins: 32 KB / 16 KB), filled with ds_add_u32.  The hard case is
// the normal one here -- bars, black frames, grey chroma: every sample of a
// wave in one bin -- and is met twice:
//   merge:   a lane adds each RUN of equal neighbouring samples of its piece
//            once, with the run's length (a constant piece: 1 add, not 8 / 16);
//   copies:  the lanes of a wave spread over R addresses in R different banks,
//            so an instruction whose lanes all hit one bin serialises 64 / R
//            ways, not 64.
// (Measured alternatives: DESIGN.md section 4.)  After a frame the workgroup
// sums the R copies (one lane a bin, 16-B LDS reads), clears them, and stores
// the tile's histogram into its slab [frame][tile][bins]; stat_finalize adds
// the slabs of a plane's tiles.  No global atomics; the sums are integers, so
// the result does not depend on any order and is identical from run to run.
//
// Exactness:
//   run:    a run's length <= 16 / es <= 16 samples (the add's operand)
//   LDS bin (one copy): <= samples of a tile = 64 rows * 1024 / es <= 65,536:
//           32 bits
//   over:   per lane and frame <= 16 pieces * 8 = 128; wave <= 8,192; tile
//           <= 32,768; plane < 2^31 (below): 32 bits throughout
//   sad:    per lane and frame <= 16 pieces * 8 samples * 65,535 < 2^23.1
//           (v_sad_u16 / v_sad_u8 into 32 bits); wave (butterfly, 32 bits)
//           < 2^29.1; tile and plane in 64 bits: a plane of < 2^31 samples
//           gives < 2^47
//   bin:    hist[k][p][v] <= samples of the plane, and the entry point
//           refuses planes of 2^31 samples or more: 32 bits
// A bin is 32 bits wide everywhere: no 16-bit or float counter exists.
#include <algorithm>
#include <cstdlib>

#include "analysis_dev.hpp"
#include "analysis_host.hpp"

namespace pp {

constexpr int kStLaneBytes = 16;   // one load per lane and piece
constexpr int kStLanes = 64;       // a wave's span of a row
constexpr int kStWaves = 4;        // waves per workgroup
constexpr int kStLaneRows = 16;    // rows of a tile one wave holds: pieces per lane
constexpr int kStTileRows = kStWaves * kStLaneRows;
constexpr int kStTileBytes = kStLanes * kStLaneBytes;
constexpr int kStGroup = 4;        // pieces (loads) in flight per lane
constexpr int kStFrames = 16;      // frames a workgroup walks over its tile

// ablation bits (PIXPATH_STATS_ABL, ablation build only)
constexpr int kStAblNoMerge = 1;   // one add per sample
constexpr int kStAblNoCopies = 2;  // every lane on copy 0
constexpr int kStAblUniform = 4;   // a piece uniform over the wave: one add by lane 0

struct StatAux {
    uint64_t sad;
    uint32_t over, pad;
};

struct StatPlane {
    const uint8_t *data, *prev;  // prev: the frame before frame 0 (any valid frame when there is none)
    int64_t ls, fs, pls;
    int rb, ph;  // bytes of a row that count; rows
    int tx;      // tiles across a row
    int pad;
};

struct StatArgs {
    StatPlane pl[3];
    int tile0[4];       // first tile of a plane within a frame; [3] = tiles
    int nframes, chunks;
    int64_t total;      // chunks * tiles
    uint32_t *phist;    // [nframes][tiles][bins]
    StatAux *paux;      // [nframes][tiles]
    int abl;
};

template <int ES, bool ALIGNED, bool RAGGED, bool SAD>
__device__ __forceinline__ void stat_unit(const StatArgs &a, int chunk, int tile, uint32_t *hist, uint32_t *s_sad,
                                          uint32_t *s_over) {
    constexpr int BINS = ES == 2 ? 1024 : 256;
    constexpr int R = ES == 2 ? 8 : 16;
    constexpr int SPP = kStLaneBytes / ES;  // samples per piece
    const int abl = PP_ABLATE(a.abl);
    const int p = plane_of_tile(a.tile0, tile);
    const StatPlane &P = a.pl[p];
    const int t = tile - a.tile0[p];
    const int band = t / P.tx, tx = t - band * P.tx;
    const int rb = P.rb, ph = P.ph;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = tx * kStTileBytes + lane * kStLaneBytes;  // byte column of the lane's pieces
    const int r0 = band * kStTileRows + wave * kStLaneRows;  // the wave's first row
    const int nrows = min(max(ph - r0, 0), kStLaneRows);     // and how many it has (wave-uniform)
    const int nb = min(max(rb - c, 0), kStLaneBytes);        // bytes of a piece inside the row
    const int nvs = nb / ES;                                 // samples of a piece that count
    const int copy = (abl & kStAblNoCopies) ? 0 : lane & (R - 1);
    const int f0 = chunk * kStFrames, f1 = min(a.nframes, f0 + kStFrames);
    // one piece of a frame: zero where it lies outside the plane or (RAGGED) in the pitch padding
    auto piece = [&](uint32_t q[4], __amdgpu_buffer_rsrc_t rs, const uint8_t *base, int64_t ls, int row, int nb) {
        load_piece<uint8_t, ALIGNED>(q, rs, base, ls, row, ph, c, rb, row < ph && nb > 0);
        if constexpr (RAGGED && ALIGNED) mask_piece(q, nb);
    };

    uint32_t pv[kStLaneRows][4];
    if constexpr (SAD) {
        const uint8_t *pb = f0 > 0 ? P.data + (int64_t)(f0 - 1) * P.fs : P.prev;
        const int64_t pls = f0 > 0 ? P.ls : P.pls;
        const auto prs = plane_rsrc<ALIGNED>(pb, ph, pls, rb);
#pragma unroll
        for (int u = 0; u < kStLaneRows; ++u) piece(pv[u], prs, pb, pls, r0 + u, nb);
    }

    for (int f = f0; f < f1; ++f) {
        const uint8_t *base = P.data + (int64_t)f * P.fs;
        const int64_t ls = P.ls;
        // the lane's extent is frame-invariant: recompute its predicates per frame
        // (a few VALU compares) instead of holding every one as an SGPR mask
        int nbf = nb, nvf = nvs;
        asm volatile("" : "+v"(nbf), "+v"(nvf));
        const auto rs = plane_rsrc<ALIGNED>(base, ph, ls, rb);
        uint32_t sad = 0, over = 0;
#pragma unroll
        for (int g = 0; g < kStLaneRows; g += kStGroup) {
            uint32_t q[kStGroup][4];
#pragma unroll
            for (int u = 0; u < kStGroup; ++u) piece(q[u], rs, base, ls, r0 + g + u, nbf);
#pragma unroll
            for (int u = 0; u < kStGroup; ++u) {
                if constexpr (SAD) {
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        if constexpr (ES == 2) sad = __builtin_amdgcn_sad_u16(q[u][d], pv[g + u][d], sad);
                        else sad = __builtin_amdgcn_sad_u8(q[u][d], pv[g + u][d], sad);
                        pv[g + u][d] = q[u][d];
                    }
                }
                if (g + u >= nrows) continue;  // wave-uniform: the row lies below the plane
                if (abl & kStAblUniform) {
                    const uint32_t first = __builtin_amdgcn_readfirstlane(q[u][0]);
                    const uint32_t v = ES == 2 ? first & 0xffffu : first & 0xffu;
                    const bool same = nvf == SPP && q[u][0] == first && q[u][1] == first && q[u][2] == first &&
                                      q[u][3] == first && first == v * (ES == 2 ? 0x00010001u : 0x01010101u);
                    if (__builtin_amdgcn_ballot_w64(same) == ~0ull) {
                        if (lane == 0) {
                            if (ES == 1 || v < (uint32_t)BINS)
                                __hip_atomic_fetch_add(&hist[v * R], (uint32_t)(64 * SPP), __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                            else
                                over += 64 * SPP;
                        }
                        continue;
                    }
                }
                uint32_t s[SPP];
#pragma unroll
                for (int j = 0; j < SPP; ++j) {
                    if constexpr (ES == 2) s[j] = (j & 1) ? q[u][j >> 1] >> 16 : q[u][j >> 1] & 0xffffu;
                    else s[j] = (q[u][j >> 2] >> (8 * (j & 3))) & 0xffu;
                }
                int nv = nvf;
                if constexpr (RAGGED) asm volatile("" : "+v"(nv));
                uint32_t cnt = 0;  // length of the run that ends at sample j
#pragma unroll
                for (int j = 0; j < SPP; ++j) {
                    const bool valid = RAGGED ? j < nv : nv > 0;
                    bool last = j == SPP - 1 || s[j + (j < SPP - 1)] != s[j] || (RAGGED && j + 1 >= nv);
                    if (abl & kStAblNoMerge) last = true;
                    ++cnt;
                    if (valid && last) {
                        if (ES == 1 || s[j] < (uint32_t)BINS)
                            __hip_atomic_fetch_add(&hist[s[j] * R + copy], cnt, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_WORKGROUP);
                        else
                            over += cnt;
                    }
                    cnt = last ? 0 : cnt;
                }
            }
        }
        sad = wave_sum(sad);
        over = wave_sum(over);
        __syncthreads();  // every add of this frame has landed; the previous frame's sums have been read
        if (lane == 0) { s_sad[wave] = sad; s_over[wave] = over; }
        // a lane a bin: sum the copies, clear them, store the tile's histogram
        uint32_t *slab = a.phist + ((int64_t)f * a.tile0[3] + tile) * BINS;
#pragma unroll
        for (int b = threadIdx.x; b < BINS; b += 256) {
            uint4 *hp = reinterpret_cast<uint4 *>(hist + b * R);
            uint32_t sum = 0;
#pragma unroll
            for (int i = 0; i < R / 4; ++i) {
                const uint4 v = hp[i];
                sum += v.x + v.y + v.z + v.w;
                hp[i] = make_uint4(0, 0, 0, 0);
            }
            slab[b] = sum;
        }
        __syncthreads();  // the copies are clear for the next frame
        if (threadIdx.x == 0) {
            StatAux x;
            x.sad = (uint64_t)s_sad[0] + s_sad[1] + s_sad[2] + s_sad[3];
            x.over = s_over[0] + s_over[1] + s_over[2] + s_over[3];
            x.pad = 0;
            a.paux[(int64_t)f * a.tile0[3] + tile] = x;
        }
    }
}

// 1-D grid over the (chunk, tile) units, chunk-major.
template <int ES, bool ALIGNED, bool RAGGED, bool SAD>
__global__ __launch_bounds__(256) void stat_kernel(const StatArgs a) {
    constexpr int WORDS = (ES == 2 ? 1024 * 8 : 256 * 16);
    __shared__ __attribute__((aligned(16))) uint32_t hist[WORDS];
    __shared__ uint32_t s_sad[kStWaves], s_over[kStWaves];
    for (int i = threadIdx.x; i < WORDS; i += 256) hist[i] = 0;
    __syncthreads();
    const int tiles = a.tile0[3];
    for (int64_t u = blockIdx.x; u < a.total; u += gridDim.x) {
        const int chunk = (int)(u / tiles);
        stat_unit<ES, ALIGNED, RAGGED, SAD>(a, chunk, (int)(u - (int64_t)chunk * tiles), hist, s_sad, s_over);
    }
}

struct StatFinal {
    int tile0[4];
    int has_prev;
};

// One workgroup per (frame, plane): a lane a bin (four with 1024 bins) over the
// slabs of the plane's tiles, then the tiles' sad and over sums.
template <int BINS>
__global__ __launch_bounds__(256) void stat_finalize(const uint32_t *phist, const StatAux *paux, StatFinal f,
                                                     uint32_t *hist, uint64_t *sad, uint32_t *over) {
    __shared__ uint64_t s_sad[kStWaves];
    __shared__ uint32_t s_over[kStWaves];
    constexpr int PER = BINS / 256;
    const int64_t k = blockIdx.x / 3;
    const int p = blockIdx.x % 3;
    const int t0 = f.tile0[p], t1 = f.tile0[p + 1], tiles = f.tile0[3];
    uint32_t acc[PER] = {};
    for (int t = t0; t < t1; ++t) {
        const uint32_t *slab = phist + (k * tiles + t) * BINS;
#pragma unroll
        for (int i = 0; i < PER; ++i) acc[i] += slab[threadIdx.x + 256 * i];
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) hist[(k * 3 + p) * BINS + threadIdx.x + 256 * i] = acc[i];
    uint64_t sd = 0;
    uint32_t ov = 0;
    for (int t = t0 + threadIdx.x; t < t1; t += 256) {
        const StatAux x = paux[k * tiles + t];
        sd += x.sad;
        ov += x.over;
    }
    sd = wave_sum(sd);
    ov = wave_sum(ov);
    if ((threadIdx.x & 63) == 0) { s_sad[threadIdx.x >> 6] = sd; s_over[threadIdx.x >> 6] = ov; }
    __syncthreads();
    if (threadIdx.x == 0) {
        over[k * 3 + p] = s_over[0] + s_over[1] + s_over[2] + s_over[3];
        if (sad) sad[k * 3 + p] = (k == 0 && !f.has_prev) ? ~uint64_t(0) : s_sad[0] + s_sad[1] + s_sad[2] + s_sad[3];
    }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_frame_stats(pp_ctx *ctx, int fmt, int w, int h, const pp_frames *src, int nframes,
                              const pp_frames *prev, uint32_t *hist, uint64_t *sad, uint32_t *over, void *stream) {
    if (!ctx || !src || !hist || !over) PP_FAIL(PP_ERR_INVALID, "null argument");
    const FmtInfo fi = fmt_info(fmt);
    if (!fi.valid) PP_FAIL(PP_ERR_INVALID, "unknown pixel format %d", fmt);
    if (fi.packed) PP_FAIL(PP_ERR_INVALID, "packed format %d: unpack it first (pp_unpack_execute)", fmt);
    if (w < 1 || h < 1) PP_FAIL(PP_ERR_INVALID, "frame %dx%d", w, h);
    if (nframes < 0) PP_FAIL(PP_ERR_INVALID, "nframes %d < 0", nframes);
    if (!sad) prev = nullptr;
    const int es = fi.depth > 8 ? 2 : 1;
    StatArgs a{};
    bool aligned = true, ragged = false;
    int tiles = 0;
    for (int p = 0; p < 3; ++p) {
        PlaneGeom g = plane_geom(fmt, w, h, p), gp = g;
        const int64_t rb = g.rb;
        const int ph = g.ph;
        // a bin is 32 bits
        if ((int64_t)g.pw * ph >= (int64_t)1 << 31)
            PP_FAIL(PP_ERR_UNSUPPORTED, "plane %d of %lld samples (limit 2^31)", p, (long long)g.pw * ph);
        if (int e = check_plane(src, p, g, aligned)) return e;
        if (prev)
            if (int e = check_plane(prev, p, gp, aligned, 0, "prev ", true)) return e;
        const int64_t ls = g.ls, fs = g.fs, pls = prev ? gp.ls : ls;
        ragged |= (rb & 15) != 0;
        StatPlane &P = a.pl[p];
        P.data = static_cast<const uint8_t *>(src->data[p]);
        P.prev = prev ? static_cast<const uint8_t *>(prev->data[p]) : P.data;
        P.ls = ls; P.fs = fs; P.pls = pls;
        P.rb = (int)rb; P.ph = ph;
        P.tx = (int)((rb + kStTileBytes - 1) / kStTileBytes);
        a.tile0[p] = tiles;
        tiles += P.tx * ((ph + kStTileRows - 1) / kStTileRows);
    }
    a.tile0[3] = tiles;
    if (nframes == 0) return PP_OK;

    hipStream_t st = static_cast<hipStream_t>(stream);
    PP_HIP(hipSetDevice(ctx->device));
    const int bins = 1 << fi.depth;
    a.nframes = nframes;
    a.chunks = (nframes + kStFrames - 1) / kStFrames;
    a.total = (int64_t)a.chunks * tiles;
    const size_t units = (size_t)nframes * tiles;
    if (int e = grow(ctx->stat, units * ((size_t)bins * 4 + sizeof(StatAux)))) return e;
    a.phist = static_cast<uint32_t *>(ctx->stat.buf);
    a.paux = reinterpret_cast<StatAux *>(a.phist + units * bins);
    static const int abl = [] {
        const char *e = PP_KNOB("PIXPATH_STATS_ABL");
        return e ? std::atoi(e) : 0;
    }();
    a.abl = abl;

    using KFn = void (*)(const StatArgs);
    const int v = !aligned ? 0 : ragged ? 1 : 2;
#define PP_STAT_K(ES, SAD)                                                                   \
    (v == 0 ? stat_kernel<ES, false, true, SAD> : v == 1 ? stat_kernel<ES, true, true, SAD> \
                                                         : stat_kernel<ES, true, false, SAD>)
    const KFn k = es == 2 ? (sad ? PP_STAT_K(2, true) : PP_STAT_K(2, false))
                          : (sad ? PP_STAT_K(1, true) : PP_STAT_K(1, false));
#undef PP_STAT_K
    const int groups = (int)std::min<int64_t>(a.total, (int64_t)std::max(1, ctx->cus) * 8);
    hipLaunchKernelGGL(k, dim3(groups), dim3(256), 0, st, a);
    StatFinal f{};
    for (int p = 0; p < 4; ++p) f.tile0[p] = a.tile0[p];
    f.has_prev = prev != nullptr;
    if (bins == 1024)
        hipLaunchKernelGGL(stat_finalize<1024>, dim3(nframes * 3), dim3(256), 0, st, a.phist, a.paux, f, hist, sad, over);
    else
        hipLaunchKernelGGL(stat_finalize<256>, dim3(nframes * 3), dim3(256), 0, st, a.phist, a.paux, f, hist, sad, over);
    PP_HIP(hipGetLastError());
    return PP_OK;
}
