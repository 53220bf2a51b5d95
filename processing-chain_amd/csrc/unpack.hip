// Unpack kernel (gfx950): v210 -> yuv422p10le and uyvy422 -> yuv422p, the
// inverse of the CPVS packers (cpvs.hip, pp_v210_pack), with a crop window.
//
// Reads the two CPVS payloads of create_cpvs (reference lib/ffmpeg.py:1177-1201:
// `-c:v v210`, `-c:v rawvideo -pix_fmt uyvy422`) back into planar 4:2:2 -- to
// score a CPVS against its AVPVS (pp_metrics), to analyse an uncompressed SRC
// (pp_siti, luma only), and to test the packers (pack -> unpack -> equal).
// Restates libavcodec/v210dec.c (three 10-bit fields a little-endian word,
// bits 30-31 ignored, sample i at its fixed position whatever W is) and the
// uyvy422 byte order U Y0 V Y1; parity with FFmpeg's decoders is unpinned.
//
// Layout: cpvs.hip's traffic in reverse.  One workgroup (one wave) per output
// row (1-D grid over frames x window rows, XCD-remapped).  Phase 1: a lane
// loads a 16-B input chunk (6 px of v210, 8 px of uyvy422; kUnpackUnroll
// chunks in flight), splits it into samples and writes them to an LDS row
// [Y | U | V] at their window columns.  Phase 2: a lane reads a 16-B piece of
// the LDS row and stores it to its plane.  A v210 group gives 12 B of Y and
// 6 B of each chroma plane, no whole output granule, so the row is re-laid-out
// through LDS rather than by lanes owning several groups: every global load
// and store instruction then covers consecutive 16-B granules across the
// lanes, and a window at any even x keeps the same loads and stores (only the
// LDS writes go sample by sample).  Algorithmic bytes = packed window rows read
// once + planar window written once; no intermediate in HBM.
// Every path choice is a predicate of unpack_plan.hpp.
#include <type_traits>

#include "common.hpp"
#include "unpack_plan.hpp"

namespace pp {

struct UnpackArgs {
    const uint8_t *src;
    int64_t sls, sfs;
    uint8_t *dst[3];
    int64_t dls[3], dfs[3];
    int64_t line_bytes;  // bytes of a source line that hold samples
    int x, y, w, h, cw;  // window; chroma width
    int q0, nq;          // first chunk of the window, chunks
    int ny, nc;          // pieces of a luma / chroma row (nc = 0: luma only)
    int src_vec, grid;
    int dst_vec[3];
};

// Chunk q of a line: one 16-B load, or byte by byte (pointer or pitch off the
// 16-B grid), bytes past the line's samples reading 0.
__device__ inline uint4 load_chunk(const uint8_t *row, int q, bool vec, int64_t line_bytes) {
    if (vec) return reinterpret_cast<const uint4 *>(row)[q];
    uint32_t wd[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t b = (int64_t)q * 16 + i;
        uint32_t v = 0;
        if (unpack_byte_in(b, line_bytes)) v = row[b];
        wd[i >> 2] |= v << (8 * (i & 3));
    }
    return uint4{wd[0], wd[1], wd[2], wd[3]};
}

template <bool V210>
__global__ __launch_bounds__(kUnpackLanes) void unpack_kernel(const UnpackArgs a) {
    using T = typename std::conditional<V210, uint16_t, uint8_t>::type;
    constexpr int PX = unpack_px(V210), CPX = PX / 2;
    constexpr int ES = unpack_es(V210), PER = 16 / ES;
    extern __shared__ uint4 lds_raw[];
    T *ly = reinterpret_cast<T *>(lds_raw);
    T *lu = ly + a.ny * PER, *lv = lu + a.nc * PER;
    const int unit = xcd_remap(blockIdx.x, gridDim.x);
    const int frame = unit / a.h, r = unit - frame * a.h;
    const int lane = threadIdx.x;
    const uint8_t *srow = a.src + frame * a.sfs + (int64_t)(a.y + r) * a.sls;
    const int cx = a.x >> 1;
    const bool chroma = a.nc != 0;  // luma only: no chroma sample leaves phase 1

    for (int base = 0; base < a.nq; base += kUnpackPass) {
        uint4 c[kUnpackUnroll];
#pragma unroll
        for (int u = 0; u < kUnpackUnroll; ++u) {
            // lanes past the end load the window's first chunk again and drop it
            const int k = base + u * kUnpackLanes + lane;
            c[u] = load_chunk(srow, a.q0 + (k < a.nq ? k : 0), a.src_vec, a.line_bytes);
        }
#pragma unroll
        for (int u = 0; u < kUnpackUnroll; ++u) {
            const int k = base + u * kUnpackLanes + lane;
            if (k >= a.nq) continue;
            const int q = a.q0 + k;
            const int s0 = q * PX - a.x, c0 = q * CPX - cx;  // window columns of the chunk's first samples
            const bool vec = unpack_chunk_vec(a.grid, q, a.x, a.w, V210);
            uint32_t Y[PX], U[CPX], V[CPX];
            if constexpr (V210) {
                const uint32_t m = 1023u;
                U[0] = c[u].x & m; Y[0] = (c[u].x >> 10) & m; V[0] = (c[u].x >> 20) & m;
                Y[1] = c[u].y & m; U[1] = (c[u].y >> 10) & m; Y[2] = (c[u].y >> 20) & m;
                V[1] = c[u].z & m; Y[3] = (c[u].z >> 10) & m; U[2] = (c[u].z >> 20) & m;
                Y[4] = c[u].w & m; V[2] = (c[u].w >> 10) & m; Y[5] = (c[u].w >> 20) & m;
                if (vec) {  // s0 is a multiple of 6: 4-B aligned words of two samples
                    uint32_t *py = reinterpret_cast<uint32_t *>(ly + s0);
                    py[0] = Y[0] | (Y[1] << 16);
                    py[1] = Y[2] | (Y[3] << 16);
                    py[2] = Y[4] | (Y[5] << 16);
                    if (chroma) {
#pragma unroll
                        for (int e = 0; e < CPX; ++e) {
                            lu[c0 + e] = static_cast<T>(U[e]);
                            lv[c0 + e] = static_cast<T>(V[e]);
                        }
                    }
                    continue;
                }
            } else {
                if (vec) {  // s0 is a multiple of 8, c0 of 4: Y as two words, U and V as one each
                    const uint32_t y0 = __builtin_amdgcn_perm(c[u].y, c[u].x, 0x07050301u);  // Y0 Y1 | Y0 Y1 of words 0, 1
                    const uint32_t y1 = __builtin_amdgcn_perm(c[u].w, c[u].z, 0x07050301u);
                    *reinterpret_cast<uint2 *>(ly + s0) = uint2{y0, y1};
                    if (chroma) {
                        const uint32_t t0 = __builtin_amdgcn_perm(c[u].y, c[u].x, 0x06020400u);  // U0 U1 V0 V1
                        const uint32_t t1 = __builtin_amdgcn_perm(c[u].w, c[u].z, 0x06020400u);  // U2 U3 V2 V3
                        *reinterpret_cast<uint32_t *>(lu + c0) = __builtin_amdgcn_perm(t1, t0, 0x05040100u);
                        *reinterpret_cast<uint32_t *>(lv + c0) = __builtin_amdgcn_perm(t1, t0, 0x07060302u);
                    }
                    continue;
                }
                const uint32_t wd[4] = {c[u].x, c[u].y, c[u].z, c[u].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    U[i] = wd[i] & 255u; Y[2 * i] = (wd[i] >> 8) & 255u;
                    V[i] = (wd[i] >> 16) & 255u; Y[2 * i + 1] = wd[i] >> 24;
                }
            }
            // sample by sample: a window off the chunk grid, the chunks across its ends, the v210 tails
#pragma unroll
            for (int e = 0; e < PX; ++e)
                if (unpack_sample_in(s0 + e, a.w)) ly[s0 + e] = static_cast<T>(Y[e]);
            if (chroma) {
#pragma unroll
                for (int e = 0; e < CPX; ++e)
                    if (unpack_sample_in(c0 + e, a.cw)) {
                        lu[c0 + e] = static_cast<T>(U[e]);
                        lv[c0 + e] = static_cast<T>(V[e]);
                    }
            }
        }
    }
    __syncthreads();

    // the LDS row as one index space of 16-B pieces over the planes written
    const int total = a.ny + 2 * a.nc;
    for (int i = lane; i < total; i += kUnpackLanes) {
        const int p = i < a.ny ? 0 : (i < a.ny + a.nc ? 1 : 2);
        const int j = p == 0 ? i : (p == 1 ? i - a.ny : i - a.ny - a.nc);
        const int n = p ? a.cw : a.w;
        const uint4 v = lds_raw[i];
        uint8_t *d = (p == 0 ? a.dst[0] + frame * a.dfs[0] + (int64_t)r * a.dls[0]
                      : p == 1 ? a.dst[1] + frame * a.dfs[1] + (int64_t)r * a.dls[1]
                               : a.dst[2] + frame * a.dfs[2] + (int64_t)r * a.dls[2]) + (int64_t)j * 16;
        const bool dvec = p == 0 ? a.dst_vec[0] : (p == 1 ? a.dst_vec[1] : a.dst_vec[2]);
        const int valid = unpack_piece_valid(j, n, ES);
        if (unpack_piece_vec(dvec, valid, ES)) {
            *reinterpret_cast<uint4 *>(d) = v;
        } else {
            for (int e = 0; e < valid; ++e) {  // selects, not a private array
                constexpr int SPD = 4 / ES;    // samples per dword
                const int dw = e / SPD;
                const uint32_t w4 = dw == 0 ? v.x : (dw == 1 ? v.y : (dw == 2 ? v.z : v.w));
                reinterpret_cast<T *>(d)[e] = static_cast<T>(w4 >> (8 * ES * (e % SPD)));
            }
        }
    }
}

int unpack_geometry(int in_fmt, int W, int H, const pp_frames *src, int x, int y, int w, int h, const pp_frames *dst,
                    int nframes, UnpackGeom *g) {
    if (!src || !dst) PP_FAIL(PP_ERR_INVALID, "null argument");
    if (nframes < 0) PP_FAIL(PP_ERR_INVALID, "nframes %d < 0", nframes);
    if (in_fmt != PP_FMT_V210 && in_fmt != PP_FMT_UYVY422)
        PP_FAIL(PP_ERR_INVALID, "unpack needs a packed format (v210 or uyvy422), got %d", in_fmt);
    const bool v210 = in_fmt == PP_FMT_V210;
    if (W < 1 || H < 1) PP_FAIL(PP_ERR_INVALID, "frame %dx%d", W, H);
    if (W & 1) PP_FAIL(PP_ERR_INVALID, "%s needs an even width, not %d", v210 ? "v210" : "uyvy422", W);
    if (w < 1 || h < 1) PP_FAIL(PP_ERR_INVALID, "window %dx%d is empty", w, h);
    if (x < 0 || y < 0 || (int64_t)x + w > W || (int64_t)y + h > H)
        PP_FAIL(PP_ERR_INVALID, "window %dx%d at (%d,%d) exceeds the frame %dx%d", w, h, x, y, W, H);
    if (x & 1) PP_FAIL(PP_ERR_INVALID, "window x %d must be even (a chroma sample spans two pixels)", x);
    const int es = unpack_es(v210), cw = (w + 1) / 2;
    const int64_t line = unpack_line_bytes(W, v210), sls = src->linesize[0];
    if (!src->data[0]) PP_FAIL(PP_ERR_INVALID, "null source data");
    if (v210 ? (sls < line || (sls & 3)) : sls < line)
        PP_FAIL(PP_ERR_INVALID, "%s source linesize %lld: need %s>= %lld", v210 ? "v210" : "uyvy422", (long long)sls,
                v210 ? "a multiple of 4 " : "", (long long)line);
    if (!dst->data[0]) PP_FAIL(PP_ERR_INVALID, "null destination luma");
    if (!dst->data[1] != !dst->data[2])
        PP_FAIL(PP_ERR_INVALID, "only one chroma destination given (both, or neither for luma only)");
    g->luma_only = !dst->data[1];
    for (int p = 0; p < (g->luma_only ? 1 : 3); ++p) {
        const int pw = p ? cw : w;
        if (dst->linesize[p] < (int64_t)pw * es) PP_FAIL(PP_ERR_INVALID, "destination plane %d: short linesize", p);
        if (((uintptr_t)dst->data[p] | (uint64_t)dst->linesize[p] | (uint64_t)dst->frame_stride[p]) & (es - 1))
            PP_FAIL(PP_ERR_INVALID, "destination plane %d: 16-bit samples off the 2-byte grid", p);
    }
    g->v210 = v210;
    g->empty = nframes == 0;
    if (g->empty) return PP_OK;
    g->W = W; g->H = H; g->x = x; g->y = y; g->w = w; g->h = h; g->cw = cw; g->es = es;
    g->q0 = unpack_first_chunk(x, v210);
    g->nq = unpack_last_chunk(x, w, v210) - g->q0 + 1;
    g->ny = unpack_pieces(w, es);
    g->nc = g->luma_only ? 0 : unpack_pieces(cw, es);
    g->lds = unpack_lds_bytes(w, g->luma_only ? 0 : cw, es);
    if (g->lds > kUnpackLdsMax) PP_FAIL(PP_ERR_UNSUPPORTED, "unpack: window width %d exceeds the LDS row stage", w);
    if ((int64_t)h * nframes >= (int64_t)1 << 31) PP_FAIL(PP_ERR_UNSUPPORTED, "unpack: too many rows in one call");
    g->src_vec = unpack_src_vec((uintptr_t)src->data[0], sls, src->frame_stride[0], nframes);
    g->grid = unpack_grid(x, v210);
    for (int p = 0; p < 3; ++p)
        g->dst_vec[p] = p < (g->luma_only ? 1 : 3) &&
                        unpack_dst_vec((uintptr_t)dst->data[p], dst->linesize[p], dst->frame_stride[p], nframes);
    return PP_OK;
}

}  // namespace pp

using namespace pp;

extern "C" int pp_unpack_execute(pp_ctx *ctx, int in_fmt, int W, int H, const pp_frames *src, int x, int y, int w,
                                 int h, const pp_frames *dst, int nframes, void *stream) {
    if (!ctx) PP_FAIL(PP_ERR_INVALID, "null argument");
    UnpackGeom g;
    const int rc = unpack_geometry(in_fmt, W, H, src, x, y, w, h, dst, nframes, &g);
    if (rc || g.empty) return rc;
    PP_HIP(hipSetDevice(ctx->device));
    UnpackArgs a{};
    a.src = static_cast<const uint8_t *>(src->data[0]);
    a.sls = src->linesize[0];
    a.sfs = src->frame_stride[0];
    for (int p = 0; p < (g.luma_only ? 1 : 3); ++p) {
        a.dst[p] = static_cast<uint8_t *>(dst->data[p]);
        a.dls[p] = dst->linesize[p];
        a.dfs[p] = dst->frame_stride[p];
        a.dst_vec[p] = g.dst_vec[p];
    }
    a.line_bytes = unpack_line_bytes(W, g.v210);
    a.x = x; a.y = y; a.w = w; a.h = h; a.cw = g.cw;
    a.q0 = g.q0; a.nq = g.nq; a.ny = g.ny; a.nc = g.nc;
    a.src_vec = g.src_vec;
    a.grid = g.grid;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(h * nframes));
    if (g.v210)
        hipLaunchKernelGGL((unpack_kernel<true>), grid, dim3(kUnpackLanes), g.lds, st, a);
    else
        hipLaunchKernelGGL((unpack_kernel<false>), grid, dim3(kUnpackLanes), g.lds, st, a);
    PP_HIP(hipGetLastError());
    return PP_OK;
}
