// Banding detection of a luma sequence (spec PP-BAND-1) on gfx950:
// for every shown frame and each of five scales the histogram of the contrast
// value Q of its positions.  The pooling is host arithmetic
// (pixpath/banding.py).  The measure is modelled on CAMBI (Tandon et al., PCS
// 2021) as recalled and defined by the spec's text alone; parity with libvmaf's
// CAMBI is unpinned: no libvmaf exists to compare with.
//
// A level of the workspace holds one 16-bit code per position: y_s in bits
// 0 .. 9 and bit 15 set where the mask m_s is 0, so a masked sample of value
// v + d is the code v + d itself, and neither an unmasked sample nor the
// code kBdOutside the contrast kernel puts around the plane ever equals one.
//
// Three kernels per launch of up to kFrameMap frames:
//   banding_prep      steps 1 - 3: a workgroup takes a tile of 32 rows x 64
//                     columns, computes y0 of the tile and a margin of 3 (4 to
//                     the right and below) into LDS from clamped element loads,
//                     the flags z from that, and the 7 x 7 sums of z as seven
//                     row sums per lane shared by its 8 consecutive rows.
//                     Element loads serve every pointer and pitch alike.
//   banding_down      step 4, once per scale: a lane per position of scale
//                     s + 1 reads the nine codes of its 3 x 3 neighbourhood
//                     (clamped), takes mode3 by counting, each value against
//                     the nine, and keeps the mask bit of the centre.  All
//                     scales together read 3 codes per sample of scale 0.
//   banding_contrast  steps 5 and 6, all scales in one grid: a workgroup owns
//                     kBdChunk tiles of 32 x 32 positions of one (frame, scale)
//                     and a sub-histogram in LDS.  A tile without a masked
//                     position is counted into bin 0 from the lanes' own codes
//                     and nothing else is loaded.  Otherwise the tile and a
//                     margin of W / 2 go to LDS (at most 94 x 94 codes) and a
//                     lane walks the W x W window of each of its four
//                     positions: per sample t = min(7 (c - v + 4), 63) and
//                     acc += 1 << t in 64 bits, nine 7-bit counters of one
//                     window row (a row holds at most 63 <= 127 samples; bit 63
//                     collects every sample outside v - 4 .. v + 4 and falls
//                     off the top), unpacked into nine 32-bit counts after
//                     each row.  That is five VALU instructions a sample,
//                     W^2 samples a masked position, none for an unmasked one.
//
// Q: num = 1024 k n_0 n_k <= 2^34 and den = (n_0 + n_k) W^2 < 2^25 are exact
// integers (64 and 32 bits); q = floor(double(num) / double(den)).  Both
// convert exactly, the IEEE quotient is below 2^11 and off by less than 2^-42,
// and a quotient that is no integer lies at least 1 / den > 2^-25 from one, so
// the floor is the integer quotient's.
//
// Histogram: bin 0 is the hard case (every unmasked position, every constant
// frame) and takes no atomic: a wave counts its lanes with Q = 0 by ballot
// into a register.  The other bins are ds_add_u32 on kBdCopies copies per bin,
// as stats.hip's.  A workgroup adds its non-empty bins to the result with
// integer atomics after its last tile; the result is cleared first.  Integer
// sums do not depend on any order: two runs give the same bits.
#include <algorithm>

#include "analysis_dev.hpp"
#include "analysis_host.hpp"

namespace pp {

constexpr int kBdScales = 5;
constexpr int kBdBins = 1024;
constexpr int kBdMaskRows = 32, kBdMaskCols = 64;  // a tile of banding_prep
constexpr int kBdTile = 32;                        // rows and columns of a tile of banding_contrast
constexpr int kBdMaxWin = 63;
constexpr int kBdSpan = kBdTile + kBdMaxWin - 1;   // the largest tile with its margin
constexpr int kBdCopies = 4;                       // LDS copies of a bin
constexpr int kBdChunk = 4;                        // tiles a workgroup walks before it adds its bins
constexpr uint32_t kBdUnmasked = 0x8000u;          // bit of a code: m_s = 0
constexpr uint32_t kBdOutside = 0x8000u;           // code of a window sample outside the plane
constexpr uint32_t kBdNone = 0xffffu;              // a lane's position outside the plane

struct BdArgs {
    const uint8_t *src;
    int64_t ls, fs;
    int w[kBdScales], h[kBdScales];
    int64_t off[kBdScales], frame;  // codes before level s of a frame; codes of a frame
    uint16_t *ws;                   // [nk][frame]
    int tx[kBdScales];              // contrast tiles across
    int unit0[kBdScales + 1];       // first workgroup of scale s within a frame; [5] = workgroups of a frame
    int nk, window;
    int tvi[4];
    uint32_t *hist;                 // [nk][5][1024]
    int32_t idx[kFrameMap];         // source frame of shown frame k
};

template <typename T>
__device__ __forceinline__ uint32_t bd_u(const uint8_t *base, int64_t ls, int i, int j) {
    const uint32_t x = reinterpret_cast<const T *>(base + (int64_t)i * ls)[j];
    return sizeof(T) == 1 ? x << 2 : min(x, 1023u);
}

// grid (tiles of 32 x 64, shown frames)
template <typename T>
__global__ __launch_bounds__(256) void banding_prep(const BdArgs a) {
    constexpr int YR = kBdMaskRows + 7, YC = kBdMaskCols + 7;  // rows and columns of y0 held
    constexpr int ZR = kBdMaskRows + 6, ZC = kBdMaskCols + 6;  // and of z
    __shared__ uint16_t s_y[YR][YC + 1];
    __shared__ uint8_t s_z[ZR][ZC + 2];
    const int w = a.w[0], h = a.h[0];
    const int tx = (w + kBdMaskCols - 1) / kBdMaskCols;
    const int band = blockIdx.x / tx, tc = blockIdx.x - band * tx;
    const int i0 = band * kBdMaskRows - 3, j0 = tc * kBdMaskCols - 3;  // position of s_y[0][0]
    const uint8_t *base = a.src + (int64_t)a.idx[blockIdx.y] * a.fs;
    const int64_t ls = a.ls;
    for (int e = threadIdx.x; e < YR * YC; e += 256) {
        const int r = e / YC, c = e - r * YC, gi = i0 + r, gj = j0 + c;
        uint32_t y = kBdNone;
        if (gi >= 0 && gi < h && gj >= 0 && gj < w) {
            const int i1 = min(gi + 1, h - 1), j1 = min(gj + 1, w - 1);
            y = (bd_u<T>(base, ls, gi, gj) + bd_u<T>(base, ls, gi, j1) + bd_u<T>(base, ls, i1, gj) +
                 bd_u<T>(base, ls, i1, j1) + 2u) >> 2;
        }
        s_y[r][c] = (uint16_t)y;
    }
    __syncthreads();
    // a position inside the plane reads only neighbours inside it: c + 1 < YC and r + 1 < YR
    for (int e = threadIdx.x; e < ZR * ZC; e += 256) {
        const int r = e / ZC, c = e - r * ZC, gi = i0 + r, gj = j0 + c;
        bool z = false;
        if (gi >= 0 && gi < h && gj >= 0 && gj < w)
            z = (gj == w - 1 || s_y[r][c] == s_y[r][c + 1]) && (gi == h - 1 || s_y[r][c] == s_y[r + 1][c]);
        s_z[r][c] = z ? 1 : 0;
    }
    __syncthreads();
    // a lane: column `col`, rows r0 .. r0 + 7 of the tile; the z rows r0 .. r0 + 13, columns col .. col + 6
    const int col = threadIdx.x & 63, r0 = (threadIdx.x >> 6) * 8;
    const int gj = j0 + 3 + col;
    if (gj >= w) return;
    uint32_t hs[14];
#pragma unroll
    for (int q = 0; q < 14; ++q) {
        uint32_t s = 0;
#pragma unroll
        for (int d = 0; d < 7; ++d) s += s_z[r0 + q][col + d];
        hs[q] = s;
    }
    uint16_t *lv = a.ws + (int64_t)blockIdx.y * a.frame + a.off[0];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int gi = i0 + 3 + r0 + p;
        if (gi >= h) break;
        uint32_t s = 0;
#pragma unroll
        for (int d = 0; d < 7; ++d) s += hs[p + d];
        const uint32_t y = s_y[r0 + p + 3][col + 3];
        lv[(int64_t)gi * w + gj] = (uint16_t)(y | (s >= 25u ? 0u : kBdUnmasked));
    }
}

// grid (positions of scale s + 1 / 256, shown frames)
__global__ __launch_bounds__(256) void banding_down(const BdArgs a, int s) {
    const int ws = a.w[s], hs = a.h[s], wd = a.w[s + 1], hd = a.h[s + 1];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= wd * hd) return;
    const int i = e / wd, j = e - i * wd;
    uint16_t *f = a.ws + (int64_t)blockIdx.y * a.frame;
    const uint16_t *L = f + a.off[s];
    uint32_t v[9];
#pragma unroll
    for (int d = 0; d < 9; ++d) {
        const int gi = min(max(2 * i + d / 3 - 1, 0), hs - 1), gj = min(max(2 * j + d % 3 - 1, 0), ws - 1);
        v[d] = L[(int64_t)gi * ws + gj];
    }
    const uint32_t flag = v[4] & kBdUnmasked;  // the centre is position (2i, 2j) itself
#pragma unroll
    for (int d = 0; d < 9; ++d) v[d] &= 0x3ffu;
    // the most frequent value, the smallest on a tie: the largest of count * 1024 + (1023 - value)
    uint32_t best = 0;
#pragma unroll
    for (int d = 0; d < 9; ++d) {
        uint32_t n = 0;
#pragma unroll
        for (int o = 0; o < 9; ++o) n += v[o] == v[d] ? 1u : 0u;
        best = max(best, n * 1024u + (1023u - v[d]));
    }
    f[a.off[s + 1] + (int64_t)i * wd + j] = (uint16_t)((1023u - (best & 1023u)) | flag);
}

// One workgroup per (shown frame, scale, chunk of kBdChunk tiles), frame-major.
__global__ __launch_bounds__(256) void banding_contrast(const BdArgs a) {
    __shared__ uint16_t s_c[kBdSpan * kBdSpan];
    __shared__ __align__(16) uint32_t s_h[kBdBins * kBdCopies];
    const int upf = a.unit0[kBdScales];
    const int k = blockIdx.x / upf, u = blockIdx.x - k * upf;
    int s = 0;
    while (s < kBdScales - 1 && u >= a.unit0[s + 1]) ++s;
    const int chunk = u - a.unit0[s];
    const int w = a.w[s], h = a.h[s], tx = a.tx[s];
    const int tiles = tx * ((h + kBdTile - 1) / kBdTile);
    const uint16_t *L = a.ws + (int64_t)k * a.frame + a.off[s];
    const int W = a.window, R = W >> 1, P = kBdTile + W - 1;  // P <= kBdSpan: the entry point's range of W
    const uint32_t W2 = (uint32_t)(W * W);
    const int lane = threadIdx.x & 63, lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (int i = threadIdx.x; i < kBdBins * kBdCopies; i += 256) s_h[i] = 0;
    uint32_t zeros = 0;  // positions with Q = 0 this wave has met
    const int t1 = min(tiles, (chunk + 1) * kBdChunk);
    for (int t = chunk * kBdChunk; t < t1; ++t) {
        const int band = t / tx, i0 = band * kBdTile, j0 = (t - band * tx) * kBdTile;
        // the lane's four positions: column j0 + lx, rows i0 + ly + 8 p
        uint32_t cc[4];
        bool any = false;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int gi = i0 + ly + 8 * p, gj = j0 + lx;
            cc[p] = (gi < h && gj < w) ? (uint32_t)L[(int64_t)gi * w + gj] : kBdNone;
            any |= !(cc[p] & kBdUnmasked);
        }
        // also: every wave has left the previous tile's windows (and the bins are clear)
        if (!__syncthreads_or(any)) {
#pragma unroll
            for (int p = 0; p < 4; ++p) zeros += __popcll(__builtin_amdgcn_ballot_w64(cc[p] != kBdNone));
            continue;
        }
        for (int e = threadIdx.x; e < P * P; e += 256) {
            const int r = e / P, c = e - r * P, gi = i0 - R + r, gj = j0 - R + c;
            s_c[e] = (gi >= 0 && gi < h && gj >= 0 && gj < w) ? L[(int64_t)gi * w + gj] : (uint16_t)kBdOutside;
        }
        __syncthreads();
#pragma unroll 1
        for (int p = 0; p < 4; ++p) {
            const bool valid = cc[p] != kBdNone, masked = !(cc[p] & kBdUnmasked);
            uint32_t q = 0;
            if (masked) {
                const int v = (int)cc[p], k7 = 7 * (v - 4);
                uint32_t n[9];
#pragma unroll
                for (int d = 0; d < 9; ++d) n[d] = 0;
                const uint16_t *row = s_c + (ly + 8 * p) * P + lx;  // the window's first sample
                for (int wr = 0; wr < W; ++wr) {
                    unsigned long long acc = 0;
                    for (int b = 0; b < W; ++b) {
                        const uint32_t sh = min((uint32_t)(7 * (int)row[b] - k7), 63u);
                        acc += 1ull << sh;
                    }
#pragma unroll
                    for (int d = 0; d < 9; ++d) n[d] += (uint32_t)(acc >> (7 * d)) & 127u;
                    row += P;
                }
                const uint32_t n0 = n[4];  // >= 1: the position itself
#pragma unroll
                for (int kk = 1; kk <= 4; ++kk) {
                    if (v > a.tvi[kk - 1]) continue;
#pragma unroll
                    for (int sg = 0; sg < 2; ++sg) {
                        const uint32_t nk = sg ? n[4 - kk] : n[4 + kk];
                        if (nk == 0) continue;
                        const unsigned long long num = 1024ull * kk * n0 * nk;
                        const uint32_t den = (n0 + nk) * W2;
                        q = max(q, (uint32_t)((double)num / (double)den));
                    }
                }
                q = min(q, (uint32_t)kBdBins - 1);  // never taken (Q <= 1023): keeps the add inside the bins
            }
            zeros += __popcll(__builtin_amdgcn_ballot_w64(valid && q == 0));
            if (valid && q != 0)
                __hip_atomic_fetch_add(&s_h[q * kBdCopies + (lane & (kBdCopies - 1))], 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    if (lane == 0 && zeros)
        __hip_atomic_fetch_add(&s_h[(threadIdx.x >> 6) & (kBdCopies - 1)], zeros, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    uint32_t *out = a.hist + ((int64_t)k * kBdScales + s) * kBdBins;
    for (int b = threadIdx.x; b < kBdBins; b += 256) {
        const uint4 c4 = *reinterpret_cast<const uint4 *>(s_h + b * kBdCopies);
        const uint32_t sum = c4.x + c4.y + c4.z + c4.w;
        if (sum) atomicAdd(out + b, sum);
    }
}

}  // namespace pp

using namespace pp;

extern "C" int pp_banding(pp_ctx *ctx, int bitdepth, int w, int h, const void *src, int64_t src_linesize,
                          int64_t src_frame_stride, int nsrc, const int32_t *index, int n, int window,
                          const uint16_t *tvi, uint32_t *hist, void *stream) {
    if (!ctx || !src || !hist) PP_FAIL(PP_ERR_INVALID, "null argument");
    LumaPlanes lp;
    if (int e = luma_open(lp, bitdepth, w, h)) return e;
    if (n < 0) PP_FAIL(PP_ERR_INVALID, "n %d < 0", n);
    if (nsrc < 0) PP_FAIL(PP_ERR_INVALID, "nsrc %d < 0", nsrc);
    if (window < 3 || window > kBdMaxWin || !(window & 1))
        PP_FAIL(PP_ERR_INVALID, "window %d (odd, 3 .. %d)", window, kBdMaxWin);
    if (int e = luma_plane(lp, src, src_linesize, src_frame_stride, "src ")) return e;
    if (int e = luma_close(lp)) return e;
    if (int e = check_frame_map(index, n, nsrc, kIndexMap)) return e;
    const int es = lp.es;
    if (n == 0) return PP_OK;

    hipStream_t st = static_cast<hipStream_t>(stream);
    PP_HIP(hipSetDevice(ctx->device));
    BdArgs a{};
    a.src = static_cast<const uint8_t *>(src);
    a.ls = src_linesize; a.fs = src_frame_stride;
    a.window = window;
    for (int k = 0; k < 4; ++k) a.tvi[k] = tvi ? tvi[k] : 1023;
    int64_t codes = 0;
    for (int s = 0; s < kBdScales; ++s) {
        a.w[s] = s ? (a.w[s - 1] + 1) / 2 : w;
        a.h[s] = s ? (a.h[s - 1] + 1) / 2 : h;
        a.off[s] = codes;
        codes += ((int64_t)a.w[s] * a.h[s] + 7) & ~int64_t(7);  // every level on the 16-B grid
        a.tx[s] = (a.w[s] + kBdTile - 1) / kBdTile;
        const int64_t tiles = (int64_t)a.tx[s] * ((a.h[s] + kBdTile - 1) / kBdTile);
        a.unit0[s + 1] = a.unit0[s] + (int)((tiles + kBdChunk - 1) / kBdChunk);
    }
    a.frame = codes;
    const int per = frames_per_launch(n, codes * 2);
    if (int e = grow(ctx->bnd, (size_t)per * (size_t)codes * 2)) return e;
    a.ws = static_cast<uint16_t *>(ctx->bnd.buf);
    const unsigned ptiles = (unsigned)(((w + kBdMaskCols - 1) / kBdMaskCols) * (int64_t)((h + kBdMaskRows - 1) / kBdMaskRows));
    // launches on one stream run in order, so they share the workspace
    const int rc = each_launch(n, per, [&](int k0, int nk) -> int {
        BdArgs b = a;
        b.nk = nk;
        fill_map(b.idx, index, k0, nk);
        b.hist = hist + (int64_t)k0 * kBdScales * kBdBins;
        PP_HIP(hipMemsetAsync(b.hist, 0, sizeof(uint32_t) * (size_t)b.nk * kBdScales * kBdBins, st));
        if (es == 2) hipLaunchKernelGGL(banding_prep<uint16_t>, dim3(ptiles, b.nk), dim3(256), 0, st, b);
        else hipLaunchKernelGGL(banding_prep<uint8_t>, dim3(ptiles, b.nk), dim3(256), 0, st, b);
        for (int s = 0; s + 1 < kBdScales; ++s)
            hipLaunchKernelGGL(banding_down, dim3((unsigned)(((int64_t)a.w[s + 1] * a.h[s + 1] + 255) / 256), b.nk),
                               dim3(256), 0, st, b, s);
        // far below 2^31 workgroups for planes inside the 2 GiB range and kFrameMap frames
        hipLaunchKernelGGL(banding_contrast, dim3((unsigned)((int64_t)b.nk * a.unit0[kBdScales])), dim3(256), 0, st, b);
        return PP_OK;
    });
    if (rc) return rc;
    PP_HIP(hipGetLastError());
    return PP_OK;
}
