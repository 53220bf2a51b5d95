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
// byte loads and explicit bounds (ALIGNED = false), equal results.
#include <algorithm>
#include <cstdlib>

#include "common.hpp"
#include "device.hpp"
#include "pack_plan.hpp"

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
    const int p = tile >= a.tile0[2] ? 2 : tile >= a.tile0[1] ? 1 : 0;
    const int band = tile - a.tile0[p];
    const int rb = a.rb[p], ph = a.ph[p], trips = a.trips[p];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: the piece loop runs on scalars
    const int r0 = band * kCrcBandRows + wave * kCrcWaveRows;  // the wave's first row
    const int n = min(max(ph - r0, 0), kCrcWaveRows);          // and how many it has
    const uint8_t *base = a.data[p] + (int64_t)k * a.fs[p];
    const uint32_t ls = (uint32_t)a.ls[p];
    // a load straddling num_records reads 0 as a whole: the last row counts up
    // to its 16-B-rounded extent, which lies inside the (aligned) pitch
    const int64_t wb = ((int64_t)rb + 15) & ~int64_t(15);
    const auto rs = uniform_rsrc(base, ALIGNED ? (int)((int64_t)(ph - 1) * a.ls[p] + wb) : 0);

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
            if constexpr (ALIGNED) {
                const uint32_t voff = in ? (uint32_t)(r0 + r) * ls + (uint32_t)c : (uint32_t)kOobOff;
                const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0);
                __builtin_memcpy(q[u], &v, 16);
            } else {
                // every load goes to a byte of the row (clamped); the select drops the others
                const uint8_t *row = base + (int64_t)(r0 + min(r, n - 1)) * a.ls[p];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    uint32_t v = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int x = c + 4 * d + e;
                        const uint32_t s = row[min(x, rb - 1)];
                        v |= ((in && x < rb) ? s : 0u) << (8 * e);
                    }
                    q[u][d] = v;
                }
            }
            if (++t == trips) { t = 0; ++r; }
        }
#pragma unroll
        for (int u = 0; u < kCrcGroup; ++u) {
            uint32_t s1 = 0, s2 = 0;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                uint32_t v = q[u][d];
                if constexpr (RAGGED && ALIGNED) {
                    const int nb = nv[u] - 4 * d;  // bytes of this dword inside the row
                    v &= nb >= 4 ? 0xffffffffu : nb <= 0 ? 0u : (1u << (8 * nb)) - 1u;
                }
                // byte j of the piece weighs 16 - j; byte 0 is the low byte of dword 0
                s1 = __builtin_amdgcn_udot4(v, 0x01010101u, s1, false);
                s2 = __builtin_amdgcn_udot4(v, 0x0D0E0F10u - 0x04040404u * d, s2, false);
            }
            A += s1;
            B += (int64_t)wgt[u] * (int64_t)(int32_t)s1 + (int64_t)s2;
        }
    }

    uint32_t ra = A % kAdlerMod, rbm = (uint32_t)((uint64_t)B % kAdlerMod);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        ra += __shfl_xor(ra, o, 64);
        rbm += __shfl_xor(rbm, o, 64);
    }
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
        const int p = t >= f.tile0[2] ? 2 : t >= f.tile0[1] ? 1 : 0;
        const int rows_end = min((t - f.tile0[p] + 1) * kCrcBandRows, f.ph[p]);
        const int64_t rest = f.N - (f.off[p] + (int64_t)rows_end * f.rb[p]);
        const CrcPartial v = q[t];
        sa += v.a;
        sb += v.b + (uint64_t)((uint32_t)(rest % kAdlerMod) * v.a);
    }
    uint32_t ra = (uint32_t)(sa % kAdlerMod), rbm = (uint32_t)(sb % kAdlerMod);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        ra += __shfl_xor(ra, o, 64);
        rbm += __shfl_xor(rbm, o, 64);
    }
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
    const int es = !fi.packed && fi.depth > 8 ? 2 : 1;
    CrcArgs a{};
    CrcFinal f{};
    bool aligned = true, ragged = false;
    for (int p = 0; p < 3; ++p) {
        a.tile0[p] = f.tile0[p] = a.tiles;
        if (p >= npl) continue;  // no units: tile0 = tiles keeps every unit in the planes before
        const int pw = p ? ceil_rshift(w, fi.hsub) : w, ph = p ? ceil_rshift(h, fi.vsub) : h;
        const int64_t rb = fmt == PP_FMT_V210 ? v210_linesize(w) : fmt == PP_FMT_UYVY422 ? 2LL * w : (int64_t)pw * es;
        const int64_t ls = src->linesize[p], fs = src->frame_stride[p];
        if (!src->data[p]) PP_FAIL(PP_ERR_INVALID, "plane %d: null data", p);
        if (ls < rb) PP_FAIL(PP_ERR_INVALID, "plane %d: linesize %lld below the row's %lld bytes", p, (long long)ls, (long long)rb);
        if (rb >= kCrcMaxRow) PP_FAIL(PP_ERR_UNSUPPORTED, "plane %d: rows of %lld bytes (limit %lld)", p, (long long)rb, (long long)kCrcMaxRow);
        // lane offsets stay inside the 31-bit buffer range
        if ((int64_t)ph * ls >= (int64_t)kOobOff)
            PP_FAIL(PP_ERR_UNSUPPORTED, "plane %d of %lld bytes exceeds the 2 GiB buffer range", p, (long long)(ph * ls));
        aligned &= !(((uintptr_t)src->data[p] | (uint64_t)ls | (uint64_t)fs) & 15);
        ragged |= (rb & 15) != 0;
        a.data[p] = static_cast<const uint8_t *>(src->data[p]);
        a.ls[p] = ls; a.fs[p] = fs;
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
    const size_t need = sizeof(CrcPartial) * (size_t)a.total;
    if (need > ctx->crc_cap) {  // grown on demand, kept by the context (hipFree waits for earlier users)
        if (ctx->crc_buf) PP_HIP(hipFree(ctx->crc_buf));
        ctx->crc_buf = nullptr; ctx->crc_cap = 0;
        PP_HIP(hipMalloc(&ctx->crc_buf, need));
        ctx->crc_cap = need;
    }
    a.part = static_cast<CrcPartial *>(ctx->crc_buf);

    using KFn = void (*)(const CrcArgs);
    const KFn k = !aligned ? crc_kernel<false, true> : ragged ? crc_kernel<true, true> : crc_kernel<true, false>;
    const int groups = (int)std::min<int64_t>(a.total, (int64_t)std::max(1, ctx->cus) * 8);
    hipLaunchKernelGGL(k, dim3(groups), dim3(256), 0, st, a);
    hipLaunchKernelGGL(crc_finalize, dim3(nframes), dim3(64), 0, st, a.part, f, init, out);
    PP_HIP(hipGetLastError());
    return PP_OK;
}
