// Per-frame Adler-32 of a frame batch (spec PP-HASH-1) on gfx950:
// the checksum FFmpeg's framecrc muxer prints, so a listing of ours can be
// diffed against `ffmpeg -f framecrc` (parity [EXT], unpinned).
//
//   M = 65521, N bytes d_0 .. d_{N-1} of the frame's byte string, start value
//   init = (b0 << 16) | a0:
//   A = (a0 + S1) mod M                 S1 = sum d_i
//   B = (b0 + N a0 + S2) mod M          S2 = sum (N - i) d_i
//
// S1 and S2 are exact integer sums and pieces of the string combine by
//   S2(chunk || rest) = S2(chunk) + len(rest) S1(chunk) + S2(rest),
// so the string is cut into pieces that are summed independently, each
// weighted by the number of bytes that follow it: nothing is sequential.
//
// Layout: a workgroup (256 lanes, 4 waves) owns one unit = (frame, plane, band
// of kCrcBandRows rows); wave v takes the kCrcWaveRows rows v*16 .. v*16+15 of
// the band.  A lane takes 16 B of a row through a bounds-checked buffer load
// (bytes past the plane read 0; the bytes of a ragged last piece that lie past
// the row's extent are masked: they are pitch padding), and forms
//   s1 = sum d_j,  s2 = sum (16 - j) d_j      (v_dot4_u32_u8, 8 per piece)
// against constant weight words.  A wave covers 1024 B of a row per trip and
// walks its (row, trip) pieces four at a time, the four loads issued before
// the first sum.  The piece at byte c of row r of the wave's n rows of rb
// bytes has w = (n - 1 - r) rb + rb - c - 16 bytes of the wave's rows after
// its 16th byte (w >= -15: the last piece of the last row), and adds
//   s1 to A_lane,   s2 + w s1 to B_lane
// which is sum (bytes from d_j to the end of the wave's rows) d_j >= 0.
//
// Exactness (all-0xFF bytes, rb < 2^24 enforced by the entry point):
//   piece:  s1 <= 16*255 = 4080, s2 <= 136*255 = 34680: 32 bits (dot4 exact)
//   lane:   pieces <= 16 rows * rb/1024 <= 2^18; A_lane <= 2^18 * 4080 < 2^30
//           in 32 bits; w < 16 rb < 2^28, one term < 2^40, B_lane < 2^58 in
//           64 bits (v_mad_i64_i32).  A 32-bit B_lane would pass 2^32 inside
//           one 1920-byte row band.  Both are reduced mod M here.
//   wave:   64 lanes of values < M: < 2^22 (xor butterfly, 32 bits)
//   unit:   wave v's sums weigh the bytes of the waves after it:
//           (rest_v mod M) * (A_v mod M) < 2^32; four such terms in 64 bits,
//           reduced mod M: the partial is (A_unit, B_unit), both < M.
//   frame:  crc_finalize, one wave per frame, a lane per unit: (rest_u mod M)
//           * A_unit < 2^32 with rest_u = N - (end of the unit) taken mod M
//           first, summed in 64 bits over <= tiles/64 units a lane, reduced,
//           butterfly < 2^22, then b0 + (N mod M) a0 + B < 2^33 in 64 bits.
// No product is formed from unreduced operands above the lane level, so the
// 2^64 limit of a plain sum (N ~ 3.8e8 bytes) does not exist here.
// No atomics: one partial per unit, added in a fixed order (and integer
// addition mod M is order-independent anyway).
//
// Pointers, linesizes or frame strides off the 16-B grid: the same kernel with
// byte loads and explicit bounds (ALIGNED = false), equal results.  The piece
// loader, its mask, the descriptor and the butterfly: analysis_dev.hpp.
#include <algorithm>
#include <cstdlib>

#include "analysis_dev.hpp"
#include "analysis_host.hpp"

namespace pp {

constexpr int kCrcLaneBytes = 16;  // one load per lane and piece
constexpr int kCrcLanes = 64;      // a wave's span of a row: 1024 B per trip
constexpr int kCrcWaves = 4;       // waves per workgroup
constexpr int kCrcWaveRows = 16;   // rows of a band one wave sums
constexpr int kCrcBandRows = kCrcWaves * kCrcWaveRows;
constexpr int kCrcGroup = 4;       // pieces (loads) in flight per lane
constexpr uint32_t kAdlerMod = 65521;
constexpr int64_t kCrcMaxRow = 1 << 24;  // bytes of a row (see the overflow analysis)

struct CrcPartial {
    uint32_t a, b;  // S1, S2 of the unit mod M, S2 relative to the unit's end
};

struct CrcArgs {
    const uint8_t *data[3];
    int64_t ls[3], fs[3];
    int rb[3], ph[3];  // bytes of a row that count; rows
    int trips[3];      // 1024-B trips a wave makes over a row
    int tile0[3];      // first unit of a plane within a frame
    int tiles;         // units of one frame
    int64_t total;     // frames * tiles
    CrcPartial *part;  // [frames][tiles]
};

template <bool ALIGNED, bool RAGGED>
__device__ __forceinline__ void crc_unit(const CrcArgs &a, int k, int tile, CrcPartial *out) {
    __shared__ uint32_t s_a[kCrcWaves], s_b[kCrcWaves];
    const int p = plane_of_tile(a.tile0, tile);
    const int band = tile - a.tile0[p];
    const int rb = a.rb[p], ph = a.ph[p], trips = a.trips[p];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: the piece loop runs on scalars
    const int r0 = band * kCrcBandRows + wave * kCrcWaveRows;  // the wave's first row
    const int n = min(max(ph - r0, 0), kCrcWaveRows);          // and how many it has
    const uint8_t *base = a.data[p] + (int64_t)k * a.fs[p];
    const auto rs = plane_rsrc<ALIGNED>(base, ph, a.ls[p], rb);

    uint32_t A = 0;
    int64_t B = 0;
    const int total = n * trips;
    int r = 0, t = 0;  // the next piece: row of the wave, trip (wave-uniform)
    for (int i = 0; i < total; i += kCrcGroup) {
        uint32_t q[kCrcGroup][4];
        int wgt[kCrcGroup], nv[kCrcGroup];
#pragma unroll
        for (int u = 0; u < kCrcGroup; ++u) {
            const int c = (t * kCrcLanes + lane) * kCrcLaneBytes;
            const bool in = i + u < total && c < rb;
            nv[u] = in ? rb - c : 0;  // bytes of the piece inside the row (may exceed 16)
            wgt[u] = (n - 1 - r) * rb + rb - c - kCrcLaneBytes;
            load_piece<uint8_t, ALIGNED>(q[u], rs, base, a.ls[p], r0 + r, ph, c, rb, in);
            if (++t == trips) { t = 0; ++r; }
        }
#pragma unroll
        for (int u = 0; u < kCrcGroup; ++u) {
            uint32_t s1 = 0, s2 = 0;
            if constexpr (RAGGED && ALIGNED) mask_piece(q[u], nv[u]);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                // byte j of the piece weighs 16 - j; byte 0 is the low byte of dword 0
                s1 = __builtin_amdgcn_udot4(q[u][d], 0x01010101u, s1, false);
                s2 = __builtin_amdgcn_udot4(q[u][d], 0x0D0E0F10u - 0x04040404u * d, s2, false);
            }
            A += s1;
            B += (int64_t)wgt[u] * (int64_t)(int32_t)s1 + (int64_t)s2;
        }
    }

    const uint32_t ra = wave_sum(A % kAdlerMod), rbm = wave_sum((uint32_t)((uint64_t)B % kAdlerMod));
    __syncthreads();  // the previous unit's partial has been read
    if (lane == 0) { s_a[wave] = ra % kAdlerMod; s_b[wave] = rbm % kAdlerMod; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sa = 0;
        uint64_t sb = 0;
        int64_t rest = 0;  // bytes of the unit after wave v's rows
        for (int v = kCrcWaves - 1; v >= 0; --v) {
            const int nv_rows = min(max(ph - (band * kCrcBandRows + v * kCrcWaveRows), 0), kCrcWaveRows);
            sa += s_a[v];
            sb += s_b[v] + (uint64_t)((uint32_t)(rest % kAdlerMod) * s_a[v]);
            rest += (int64_t)nv_rows * rb;
        }
        out->a = sa % kAdlerMod;
        out->b = (uint32_t)(sb % kAdlerMod);
    }
}

// 1-D grid over the (frame, unit) pairs, frame-major, XCD-aware numbering as
// in metrics_kernel (neighbouring bands of a frame on one XCD).
template <bool ALIGNED, bool RAGGED>
__global__ __launch_bounds__(256) void crc_kernel(const CrcArgs a) {
    for (int64_t u = xcd_remap(blockIdx.x, gridDim.x); u < a.total; u += gridDim.x) {
        const int k = (int)(u / a.tiles);
        crc_unit<ALIGNED, RAGGED>(a, k, (int)(u - (int64_t)k * a.tiles), a.part + u);
    }
}

struct CrcFinal {
    int tile0[3], rb[3], ph[3];
    int tiles;
    int64_t off[3];  // where a plane starts in the frame's byte string
    int64_t N;       // bytes of the string
};

// One wave per frame, a lane per unit (stride 64): each unit's sums weighted
// by the bytes of the frame after it, then the start value.
__global__ __launch_bounds__(64) void crc_finalize(const CrcPartial *part, CrcFinal f, uint32_t init, uint32_t *out) {
    const int64_t k = blockIdx.x;
    const CrcPartial *q = part + k * f.tiles;
    uint64_t sa = 0, sb = 0;
    for (int t = threadIdx.x; t < f.tiles; t += 64) {
        const int p = plane_of_tile(f.tile0, t);
        const int rows_end = min((t - f.tile0[p] + 1) * kCrcBandRows, f.ph[p]);
        const int64_t rest = f.N - (f.off[p] + (int64_t)rows_end * f.rb[p]);
        const CrcPartial v = q[t];
        sa += v.a;
        sb += v.b + (uint64_t)((uint32_t)(rest % kAdlerMod) * v.a);
    }
    const uint32_t ra = wave_sum((uint32_t)(sa % kAdlerMod)), rbm = wave_sum((uint32_t)(sb % kAdlerMod));
    if (threadIdx.x == 0) {
        const uint32_t a0 = init & 0xffffu, b0 = init >> 16;
        const uint32_t A = (a0 + ra) % kAdlerMod;
        const uint64_t B = ((uint64_t)b0 + (uint64_t)(uint32_t)(f.N % kAdlerMod) * a0 + rbm) % kAdlerMod;
        out[k] = ((uint32_t)B << 16) | A;
    }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_frame_adler32(pp_ctx *ctx, int fmt, int w, int h, const pp_frames *src, int nframes, uint32_t init,
                                uint32_t *out, void *stream) {
    if (!ctx || !src || !out) PP_FAIL(PP_ERR_INVALID, "null argument");
    const FmtInfo fi = fmt_info(fmt);
    if (!fi.valid) PP_FAIL(PP_ERR_INVALID, "unknown pixel format %d", fmt);
    if (w < 1 || h < 1) PP_FAIL(PP_ERR_INVALID, "frame %dx%d", w, h);
    if (fi.packed && (w & 1))
        PP_FAIL(PP_ERR_INVALID, "%s needs an even width, not %d", fmt == PP_FMT_V210 ? "v210" : "uyvy422", w);
    if (nframes < 0) PP_FAIL(PP_ERR_INVALID, "nframes %d < 0", nframes);
    const int npl = fi.packed ? 1 : 3;
    CrcArgs a{};
    CrcFinal f{};
    bool aligned = true, ragged = false;
    for (int p = 0; p < 3; ++p) {
        a.tile0[p] = f.tile0[p] = a.tiles;
        if (p >= npl) continue;  // no units: tile0 = tiles keeps every unit in the planes before
        PlaneGeom g = plane_geom(fmt, w, h, p);
        const int64_t rb = g.rb;
        const int ph = g.ph;
        if (int e = check_plane(src, p, g, aligned)) return e;
        if (rb >= kCrcMaxRow) PP_FAIL(PP_ERR_UNSUPPORTED, "plane %d: rows of %lld bytes (limit %lld)", p, (long long)rb, (long long)kCrcMaxRow);
        ragged |= (rb & 15) != 0;
        a.data[p] = static_cast<const uint8_t *>(src->data[p]);
        a.ls[p] = g.ls; a.fs[p] = g.fs;
        a.rb[p] = f.rb[p] = (int)rb; a.ph[p] = f.ph[p] = ph;
        a.trips[p] = (int)((rb + kCrcLanes * kCrcLaneBytes - 1) / (kCrcLanes * kCrcLaneBytes));
        a.tiles += (ph + kCrcBandRows - 1) / kCrcBandRows;
        f.off[p] = f.N;
        f.N += rb * ph;
    }
    f.tiles = a.tiles;
    if (nframes == 0) return PP_OK;

    hipStream_t st = static_cast<hipStream_t>(stream);
    PP_HIP(hipSetDevice(ctx->device));
    a.total = (int64_t)nframes * a.tiles;
    if (int e = grow(ctx->crc, sizeof(CrcPartial) * (size_t)a.total)) return e;
    a.part = static_cast<CrcPartial *>(ctx->crc.buf);

    using KFn = void (*)(const CrcArgs);
    const KFn k = !aligned ? crc_kernel<false, true> : ragged ? crc_kernel<true, true> : crc_kernel<true, false>;
    const int groups = (int)std::min<int64_t>(a.total, (int64_t)std::max(1, ctx->cus) * 8);
    hipLaunchKernelGGL(k, dim3(groups), dim3(256), 0, st, a);
    hipLaunchKernelGGL(crc_finalize, dim3(nframes), dim3(64), 0, st, a.part, f, init, out);
    PP_HIP(hipGetLastError());
    return PP_OK;
}
