// Scaler plans and the fused separable polyphase kernel (gfx950).
//
// Reference semantics: FFmpeg 7.0 libswscale generic path as used by
// `scale=W:H:flags=bicubic` (lib/ffmpeg.py:992, :1038, :1213, :800) and the
// implicit `-pix_fmt` conversions (:994, :1048, :1198):
//   hScale{8,16}To15   -> 15-bit intermediates  (Σ src*hcoef) >> (8-bit: 7, N-bit: N-1), min 32767
//   yuv2planeX_8       -> clip_u8((dither<<12 + Σ inter*vcoef) >> 19)
//   yuv2planeX_10      -> clip_u10((1<<16 + Σ inter*vcoef) >> 17)
// dither = ff_dither_8x8_128[row & 7][(col + off) & 7] when a >8-bit source is
// narrowed to 8 bit (off = 3 for the V plane), flat 64 otherwise.
//
// MI355X design ("strip streaming"): one workgroup (256 lanes = 4 wave64) owns
// a TW-wide (256 unless a large downscale needs narrower) column strip of one
// plane of one frame, split vertically into a few segments, and walks it top to
// bottom in chunks of CHO output rows.  Per chunk it stages only the source
// rows not seen before (16-B vector loads -> LDS), runs the horizontal pass
// LDS->LDS into a ring of 15-bit intermediate rows (coefficients in VGPRs, one
// output column per lane), then the vertical pass ring->HBM with wave-uniform
// coefficients (scalar loads) and 4 outputs per lane (one ds_read_b64 per tap).
// Every source row is read from HBM once per strip (plus a few rows at segment
// seams and a column halo of ~taps/TW), intermediates never touch HBM, and all
// three planes of a whole frame batch go in ONE launch
// (blockIdx.x = strip x segment over the planes, blockIdx.y = frame).
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <type_traits>

#include "filters.hpp"
#include "scale_dev.hpp"

namespace pp {

// TWC: 256 when every plane uses 256-column strips (the usual case: lane =
// column, wave = row group, all row loops wave-uniform), 0 for the general
// strip width.
template <typename ST, int OUTB, int HT, int TWC>
__global__ __launch_bounds__(kThreads) void scale_kernel(const ScaleArgs a) {
    extern __shared__ __align__(16) uint16_t lds[];
    // 1-D grid of frames x tiles, XCD-aware: an XCD walks consecutive strips of
    // consecutive frames, so strip and segment halos hit its L2
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int frame = L / a.tiles;
    int t = L - frame * a.tiles;
    int p = 0;
    if (a.nplanes > 1 && t >= a.pl[1].tile_base) p = 1;
    if (a.nplanes > 2 && t >= a.pl[2].tile_base) p = 2;
    const PlaneJob &J = a.pl[p];
    t -= J.tile_base;
    const int seg = t / J.tiles_x, tx = t - seg * J.tiles_x;
    const int TW = TWC ? TWC : J.tw;
    const int x0 = tx * TW, nx = min(TW, J.dw - x0);
    const int c0 = J.tile_c0[tx], cn = J.tile_cn[tx];
    const int S = J.S;
    uint16_t *src_t = lds;                                              // [maxnew][S]
    // window of 15-bit intermediates, row pairs interleaved per column: the
    // dword [k][c] holds rows (base + 2k, base + 2k + 1) of column c, base = the
    // chunk's first source row rounded down to even (rows a chunk shares with
    // the previous one are moved down at the chunk start, so reads never wrap)
    int16_t *ring = reinterpret_cast<int16_t *>(lds + J.maxnew * S);
    uint32_t *win = reinterpret_cast<uint32_t *>(ring);
    int32_t *vcl = reinterpret_cast<int32_t *>(ring + J.ring * TW);     // [cho][vtp] chunk V tap pairs
    int32_t *vpl = vcl + J.cho * J.vtp;                                  // [cho] chunk V base rows
    const int tid = threadIdx.x;
    const ST *sbase = reinterpret_cast<const ST *>(a.src[p] + frame * a.sfs[p]);
    uint8_t *dbase = a.dst[p] + frame * a.dfs[p];

    // horizontal-pass lane mapping: one output column per lane, r_step rows at a time
    const int col = TWC ? tid : tid % TW, r_first = TWC ? 0 : tid / TW, r_step = TWC ? 1 : kThreads / TW;
    // taps as packed 16-bit pairs for v_dot2_i32_i16 (HT is 1 or even)
    constexpr int HP = HT == 1 ? 1 : HT / 2;
    v2i16 hcp[HP];
#pragma unroll
    for (int j = 0; j < HP; ++j) hcp[j] = v2i16{0, 0};
    int hbias = 0;  // 32768 * sum(coef): undoes the staging bias of 16-bit samples
    int hoff = 0;
    if (col < nx) {
        const int x = x0 + col;
        hoff = J.hpos[x] - c0;
        int hsum = 0;
        if constexpr (HT == 1) {
            const int c = J.hcoef[x];
            hcp[0] = v2i16{(int16_t)c, 0};
            hsum = c;
        } else {
#pragma unroll
            for (int j = 0; j < HP; ++j) {
                const int16_t c0_ = J.hcoef[(int64_t)x * HT + 2 * j], c1_ = J.hcoef[(int64_t)x * HT + 2 * j + 1];
                hcp[j] = v2i16{c0_, c1_};
                hsum += c0_ + c1_;
            }
        }
        if constexpr (sizeof(ST) == 2) hbias = hsum * 32768;
    }
    // vertical-pass lane mapping: 4 adjacent outputs per lane
    const int groups = TW / 4;
    const int lane_g = TWC ? (tid & 63) : tid % groups, row_first = TWC ? (tid >> 6) : tid / groups,
              row_step = TWC ? 4 : kThreads / groups;
    const int cx = lane_g * 4;
    const int vtp = J.vtp;
    (void)J.twl;

    const int y_begin = seg * J.seg_h, y_end = min(J.dh, y_begin + J.seg_h);
    constexpr int CH = 16 / sizeof(ST);
    const int cpr = (cn + CH - 1) / CH;  // 16-B chunks per staged row
    const int64_t sls = a.sls[p];
    const bool vec = a.vec_src;
    const int sw = J.sw;
    // a 16-B load that straddles num_records reads 0 as a whole, so the last
    // row counts up to its 16-B-rounded width (inside the pitch: the vector
    // path requires 16-B aligned linesizes; see pp_frames in pixpath.h)
    const int64_t last_row = std::min<int64_t>(sls, ((int64_t)sw * sizeof(ST) + 15) & ~int64_t(15));
    const __amdgpu_buffer_rsrc_t rs = uniform_rsrc(sbase, (int)((int64_t)(J.sh - 1) * sls + last_row));
    const int cbyte = c0 * (int)sizeof(ST);
    // byte offset of chunk `id` of rows [from, ...) (kOobOff when id >= total)
    auto chunk_off = [&](int id, int from, int total) {
        const int r = id / cpr, ch = id - r * cpr;
        const int off = (from + r) * (int)sls + cbyte + ch * 16;
        return id < total ? off : kOobOff;
    };
    // staging coordinates, fixed per lane when a row has <= 256 chunks: chunk
    // column s_ch of rows s_r0, s_r0 + s_rstep, ... (no division per chunk)
    const bool fixed = cpr <= kThreads;
    const int s_rstep = fixed ? kThreads / cpr : 1;
    const int s_r0 = fixed ? tid / cpr : 0, s_ch = fixed ? tid - s_r0 * cpr : 0;
    const bool s_on = fixed && s_r0 < s_rstep;
    const int s_lds = s_r0 * S + s_ch * CH;            // LDS sample offset of the lane's first row
    const int s_goff = s_r0 * (int)sls + cbyte + s_ch * 16;  // its byte offset within the plane, less `from` rows
    // issue the loads of chunk rows [from, hi) for this lane (first kPF rows of
    // its column); straight-line code, so the kPF loads are all in flight at once
    auto prefetch = [&](Prefetch<ST> &pf, int from, int hi_) {
        if (!vec) return;
        if (fixed) {
            const int nrow = hi_ - from;
#pragma unroll
            for (int k = 0; k < kPF; ++k) {
                const int r = s_r0 + k * s_rstep;
                pf.v[k] = bload16(rs, (s_on && r < nrow) ? s_goff + (from + k * s_rstep) * (int)sls : kOobOff);
            }
        } else {
            const int total = (hi_ - from) * cpr;
#pragma unroll
            for (int k = 0; k < kPF; ++k) pf.v[k] = bload16(rs, chunk_off(tid + k * kThreads, from, total));
        }
    };
    // write the prefetched chunks to LDS and stage any remainder synchronously
    auto commit = [&](const Prefetch<ST> &pf, int from, int hi_) {
        const int total = (hi_ - from) * cpr;
        if (!vec) {
            for (int id = tid; id < total; id += kThreads) {
                const int r = id / cpr, ch = id - r * cpr;
                const ST *g = reinterpret_cast<const ST *>(reinterpret_cast<const uint8_t *>(sbase) +
                                                           (int64_t)(from + r) * sls);
                store16<ST>(src_t + r * S + ch * CH, load16_scalar<ST>(g, c0 + ch * CH, sw));
            }
            return;
        }
        if (fixed) {
            const int nrow = hi_ - from;
            if (!s_on) return;
#pragma unroll
            for (int k = 0; k < kPF; ++k)
                if (s_r0 + k * s_rstep < nrow) store16<ST>(src_t + s_lds + k * s_rstep * S, pf.v[k]);
            for (int k = kPF; s_r0 + k * s_rstep < nrow; ++k)
                store16<ST>(src_t + s_lds + k * s_rstep * S, bload16(rs, s_goff + (from + k * s_rstep) * (int)sls));
            return;
        }
#pragma unroll
        for (int k = 0; k < kPF; ++k) {
            const int id = tid + k * kThreads;
            if (id < total) {
                const int r = id / cpr, ch = id - r * cpr;
                store16<ST>(src_t + r * S + ch * CH, pf.v[k]);
            }
        }
        for (int id = tid + kPF * kThreads; id < total; id += kThreads) {
            const int r = id / cpr, ch = id - r * cpr;
            store16<ST>(src_t + r * S + ch * CH, bload16(rs, chunk_off(id, from, total)));
        }
    };

    int next_src = J.chunk_lo[y_begin / J.cho];
    int base = next_src & ~1;  // window row 0 (even source row)
    Prefetch<ST> pf;
    // rows the first chunk needs
    int pf_from = next_src, pf_hi = J.chunk_hi[y_begin / J.cho];
    if (pf_from < J.chunk_lo[y_begin / J.cho]) pf_from = J.chunk_lo[y_begin / J.cho];
    prefetch(pf, pf_from, pf_hi);
    // one H-pass output row: taps over the staged source row at `sp` (window
    // start hoff, 4-B aligned reads, odd starts re-paired with v_alignbit)
    const int odd = hoff & 1;
    const uint32_t ash = odd * 16;
    auto hrow = [&](const uint16_t *sp) -> uint32_t {
        int acc;
        if constexpr (HT == 1) {
            acc = hbias + static_cast<int>(static_cast<int16_t>(sp[odd])) * hcp[0][0];
        } else {
            const uint32_t *sw32 = static_cast<const uint32_t *>(__builtin_assume_aligned(sp, 4));
            uint32_t w[HP + 1];
#pragma unroll
            for (int j = 0; j <= HP; ++j) w[j] = sw32[j];
            acc = dot2_acc(__builtin_bit_cast(v2i16, __builtin_amdgcn_alignbit(w[1], w[0], ash)), hcp[0], hbias);
#pragma unroll
            for (int j = 1; j < HP; ++j)
                acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2i16, __builtin_amdgcn_alignbit(w[j + 1], w[j], ash)),
                                             hcp[j], acc, false);
        }
        acc >>= a.hshift;
        return static_cast<uint32_t>(acc < 32767 ? acc : 32767) & 0xffffu;
    };
    const int nxw = TWC ? TW : nx;  // window columns written (TWC: all, harmlessly)
    for (int y0 = y_begin; y0 < y_end; y0 += J.cho) {
        const int ci = y0 / J.cho;
        const int lo = J.chunk_lo[ci], hi = J.chunk_hi[ci];
        if (next_src < lo) next_src = lo;
        const int nnew = hi - next_src;
        const int nbase = lo & ~1;
        // rows kept from the previous chunk: [nbase, next_src), as whole pairs
        const int keep = next_src > nbase ? (next_src - nbase + 1) >> 1 : 0;
        const int shift = (nbase - base) >> 1;
        // ---- commit the prefetched rows (src_t is not read by the vertical pass) ----
        if (nnew > 0) commit(pf, next_src, hi);
        __syncthreads();  // staged rows visible; every wave has left the previous vertical pass
        // ---- this chunk's vertical taps/rows: written only after the barrier above
        // (the previous vertical pass reads them), visible after the one below ----
        {
            const int ny_c = min(J.cho, y_end - y0);
            for (int i = tid; i < ny_c * vtp; i += kThreads) vcl[i] = J.vcoef2[(int64_t)y0 * vtp + i];
            for (int i = tid; i < ny_c; i += kThreads) vpl[i] = J.vbase[y0 + i] - nbase;
        }
        // ---- move the kept pairs down to the window start: each column by one
        // lane, in increasing order, so no lane reads a slot already overwritten ----
        if (shift > 0 && r_first == 0 && col < nxw) {
            for (int k = 0; k < keep; ++k) win[k * TW + col] = win[(k + shift) * TW + col];
        }
        // general strip width: other lanes of the column write new pairs that the
        // copy may still have to read (TWC: one lane per column, program order)
        if constexpr (!TWC) __syncthreads();
        base = nbase;
        // ---- horizontal pass into the window, one row pair per step -------------
        // (TWC: lanes past the strip's last column compute with zero taps and
        // write window columns the vertical pass never reads -- no divergence)
        if (nnew > 0 && col < nxw) {
            const int i0 = next_src - base;            // window row of the first new row
            const uint16_t *sp = src_t + hoff - odd;
            // a half pair at each end (its other row is kept, or not needed), full
            // pairs in between: one packed 32-bit write per two rows
            const int kf0 = (i0 + 1) >> 1, kf1 = (i0 + nnew) >> 1;
            if ((i0 & 1) && r_first == 0)  // high row of pair i0/2 (same lane as the copy above)
                reinterpret_cast<uint16_t *>(win + (i0 >> 1) * TW + col)[1] = static_cast<uint16_t>(hrow(sp));
            if (((i0 + nnew) & 1) && r_first == r_step - 1)  // low row of the last pair
                reinterpret_cast<uint16_t *>(win + kf1 * TW + col)[0] =
                    static_cast<uint16_t>(hrow(sp + (nnew - 1) * S));
            for (int k = kf0 + r_first; k < kf1; k += r_step) {
                const int ra = 2 * k - i0;             // new-row index of the pair's low row
                const uint32_t lo16 = hrow(sp + ra * S), hi16 = hrow(sp + (ra + 1) * S);
                win[k * TW + col] = lo16 | (hi16 << 16);
            }
        }
        if (nnew > 0) next_src = hi;
        __syncthreads();
        // ---- prefetch the next chunk's new rows; their loads overlap the V pass ----
        if (y0 + J.cho < y_end) {
            const int nlo = J.chunk_lo[ci + 1], nhi = J.chunk_hi[ci + 1];
            prefetch(pf, max(next_src, nlo), nhi);
        }
        // ---- vertical pass: output rows [y0, y0 + cho) --------------------------
        const int ny = min(J.cho, y_end - y0);
        for (int yy0 = row_first; yy0 < ny + row_first; yy0 += row_step) {
            int yy = yy0;
            if (TW == kTileW) yy = __builtin_amdgcn_readfirstlane(yy);
            if (yy >= ny) break;
            const int y = y0 + yy;
            const int32_t *vc = vcl + yy * vtp;
            if (cx >= nx) continue;
            int acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
            // pairs (vbase + 2j, vbase + 2j + 1) of columns cx..cx+3: one 16-B read each
            const uint4 *rp = reinterpret_cast<const uint4 *>(win + (vpl[yy] >> 1) * TW + cx);
#pragma unroll 2
            for (int j = 0; j < vtp; ++j) {
                const v2i16 cf = __builtin_bit_cast(v2i16, vc[j]);
                const uint4 q = rp[j * (TW / 4)];
                acc0 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2i16, q.x), cf, acc0, false);
                acc1 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2i16, q.y), cf, acc1, false);
                acc2 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2i16, q.z), cf, acc2, false);
                acc3 = __builtin_amdgcn_sdot2(__builtin_bit_cast(v2i16, q.w), cf, acc3, false);
            }
            const int x = x0 + cx;
            int o[4];
            if constexpr (OUTB == 8) {
                const int drow = y & 7;
                int d[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] = a.dither ? c_dither[drow][(x + j + J.dither_off) & 7] : 64;
                o[0] = (acc0 + (d[0] << 12)) >> 19;
                o[1] = (acc1 + (d[1] << 12)) >> 19;
                o[2] = (acc2 + (d[2] << 12)) >> 19;
                o[3] = (acc3 + (d[3] << 12)) >> 19;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = min(max(o[j], 0), 255);
                uint8_t *drow_p = dbase + (int64_t)y * a.dls[p];
                if (a.vec_dst && x + 3 < J.dw) {
                    *reinterpret_cast<uint32_t *>(drow_p + x) =
                        (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x + j < J.dw) drow_p[x + j] = (uint8_t)o[j];
                }
            } else {
                constexpr int sh = 11 + 16 - OUTB;
                constexpr int mx = (1 << OUTB) - 1;
                o[0] = (acc0 + (1 << (sh - 1))) >> sh;
                o[1] = (acc1 + (1 << (sh - 1))) >> sh;
                o[2] = (acc2 + (1 << (sh - 1))) >> sh;
                o[3] = (acc3 + (1 << (sh - 1))) >> sh;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = min(max(o[j], 0), mx);
                uint16_t *drow_p = reinterpret_cast<uint16_t *>(dbase + (int64_t)y * a.dls[p]);
                if (a.vec_dst && x + 3 < J.dw) {
                    uint2 v;
                    v.x = (uint32_t)o[0] | ((uint32_t)o[1] << 16);
                    v.y = (uint32_t)o[2] | ((uint32_t)o[3] << 16);
                    *reinterpret_cast<uint2 *>(drow_p + x) = v;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x + j < J.dw) drow_p[x + j] = (uint16_t)o[j];
                }
            }
        }
    }
}

// planarCopyWrapper (same subsampling, same or wider depth): 8 samples per lane.
__global__ __launch_bounds__(256) void copy_widen_kernel(const uint8_t *src, int64_t sls, int64_t sfs, int sbytes,
                                                         uint8_t *dst, int64_t dls, int64_t dfs, int dbytes,
                                                         int w, int h, int shift) {
    const int frame = blockIdx.z;
    const int y = blockIdx.y;
    const uint8_t *s = src + frame * sfs + (int64_t)y * sls;
    uint8_t *d = dst + frame * dfs + (int64_t)y * dls;
    for (int x = (blockIdx.x * 256 + threadIdx.x) * 8; x < w; x += gridDim.x * 256 * 8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (x + e >= w) break;
            const int v = sbytes == 1 ? s[x + e] : reinterpret_cast<const uint16_t *>(s)[x + e];
            if (dbytes == 1)
                d[x + e] = (uint8_t)v;
            else
                reinterpret_cast<uint16_t *>(d)[x + e] = (uint16_t)(v << shift);
        }
    }
}

// yuv422pToUyvyWrapper: interleave U Y V Y (8-bit); one lane writes 16 bytes.
__global__ __launch_bounds__(256) void interleave_uyvy_kernel(const uint8_t *Y, const uint8_t *U, const uint8_t *V,
                                                              int64_t yls, int64_t uls, int64_t vls, int64_t yfs,
                                                              int64_t ufs, int64_t vfs, uint8_t *dst, int64_t dls,
                                                              int64_t dfs, int w, int h) {
    const int frame = blockIdx.z, y = blockIdx.y;
    const uint8_t *yr = Y + frame * yfs + (int64_t)y * yls;
    const uint8_t *ur = U + frame * ufs + (int64_t)y * uls;
    const uint8_t *vr = V + frame * vfs + (int64_t)y * vls;
    uint8_t *d = dst + frame * dfs + (int64_t)y * dls;
    const int pairs = (w + 1) / 2;
    for (int q = (blockIdx.x * 256 + threadIdx.x) * 4; q < pairs; q += gridDim.x * 256 * 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = q + e;
            if (i >= pairs) break;
            d[4 * i + 0] = ur[i];
            d[4 * i + 1] = yr[2 * i];
            d[4 * i + 2] = vr[i];
            d[4 * i + 3] = (2 * i + 1 < w) ? yr[2 * i + 1] : 0;
        }
    }
}


template <typename ST, int OUTB, int TWC>
KernelFn pick_ht_tw(int ht) {
    switch (ht) {
    case 1: return scale_kernel<ST, OUTB, 1, TWC>;
    case 2: return scale_kernel<ST, OUTB, 2, TWC>;
    case 4: return scale_kernel<ST, OUTB, 4, TWC>;
    case 6: return scale_kernel<ST, OUTB, 6, TWC>;
    case 8: return scale_kernel<ST, OUTB, 8, TWC>;
    case 12: return scale_kernel<ST, OUTB, 12, TWC>;
    case 16: return scale_kernel<ST, OUTB, 16, TWC>;
    case 24: return scale_kernel<ST, OUTB, 24, TWC>;
    case 32: return scale_kernel<ST, OUTB, 32, TWC>;
    default: return nullptr;
    }
}

template <typename ST, int OUTB>
KernelFn pick_ht(int ht, bool tw256) {
    return tw256 ? pick_ht_tw<ST, OUTB, kTileW>(ht) : pick_ht_tw<ST, OUTB, 0>(ht);
}

} // namespace pp

// ---------------------------------------------------------------------------
// A plan: the planner's layout (scale_plan.cpp: every decision and table, made
// on the host) and what lives on the device.
struct pp_scale_plan {
    pp_ctx *ctx = nullptr;                  // NULL: host-only plan (introspection; nothing uploaded, cannot execute)
    std::unique_ptr<pp::ScaleLayout> lay;   // its job / fjob table pointers are bound to `dev`
    void *dev = nullptr;                    // the layout's table blob, one allocation
    void *scratch = nullptr;                // planar temp of the two-launch CHAIN / GENERIC_UYVY paths
    int scratch_frames = 0;
    pp_scale_plan *stage2 = nullptr;        // CHAIN: the plans of the layout's stage2 / luma layouts
    pp_scale_plan *luma = nullptr;
    hipStream_t side = nullptr;             // CHAIN with `luma`: the luma launch's stream when the two launches overlap
    hipEvent_t fork = nullptr, join = nullptr;
};

namespace {

using pp::KernelFn;
using pp::PlaneJob;
using pp::ScaleArgs;
using pp::ScaleLayout;

struct PlanFree {
    void operator()(pp_scale_plan *P) const { (void)pp_scale_plan_destroy(P); }
};

// A layout (and its nested ones) as a plan.  With a context the tables go to
// the device -- one allocation, one copy -- and the jobs are bound to them.
int make_plan(pp_ctx *ctx, std::unique_ptr<ScaleLayout> lay, pp_scale_plan **out) {
    std::unique_ptr<pp_scale_plan, PlanFree> P(new pp_scale_plan());
    P->ctx = ctx;
    P->lay = std::move(lay);
    ScaleLayout &L = *P->lay;
    if (L.stage2)
        if (int rc = make_plan(ctx, std::move(L.stage2), &P->stage2)) return rc;
    if (L.luma)
        if (int rc = make_plan(ctx, std::move(L.luma), &P->luma)) return rc;
    if (ctx && !L.blob.empty()) {
        PP_HIP(hipSetDevice(ctx->device));
        PP_HIP(hipMalloc(&P->dev, L.blob.size()));
        PP_HIP(hipMemcpy(P->dev, L.blob.data(), L.blob.size(), hipMemcpyHostToDevice));
        pp::bind(L, P->dev);
        std::vector<uint8_t>().swap(L.blob);  // the host copy is not needed again
    }
    *out = P.release();
    return PP_OK;
}

}  // namespace

extern "C" int pp_scale_plan_create(pp_ctx *ctx, int src_fmt, int sw, int sh, int dst_fmt, int dw, int dh,
                                    int flags, double p0, double p1, pp_scale_plan **out) {
    if (!out) PP_FAIL(PP_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<ScaleLayout> lay;
    if (int rc = pp::plan_layout(src_fmt, sw, sh, dst_fmt, dw, dh, flags, p0, p1, &lay)) return rc;
    return make_plan(ctx, std::move(lay), out);
}

extern "C" int pp_scale_chain_plan_create(pp_ctx *ctx, int src_fmt, int sw, int sh, int dst_fmt, int dw, int dh,
                                          int flags, double p0, double p1, pp_scale_plan **out) {
    if (!out) PP_FAIL(PP_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<ScaleLayout> lay;
    if (int rc = pp::plan_chain_layout(src_fmt, sw, sh, dst_fmt, dw, dh, flags, p0, p1, &lay)) return rc;
    return make_plan(ctx, std::move(lay), out);
}

extern "C" int pp_scale_plan_destroy(pp_scale_plan *P) {
    if (!P) return PP_OK;
    if (P->stage2) (void)pp_scale_plan_destroy(P->stage2);
    if (P->luma) (void)pp_scale_plan_destroy(P->luma);
    if (P->side) (void)hipStreamDestroy(P->side);
    if (P->fork) (void)hipEventDestroy(P->fork);
    if (P->join) (void)hipEventDestroy(P->join);
    if (P->dev) (void)hipFree(P->dev);
    if (P->scratch) (void)hipFree(P->scratch);
    delete P;
    return PP_OK;
}

extern "C" int pp_scale_plan_path(const pp_scale_plan *P) {
    if (!P) PP_FAIL(PP_ERR_INVALID, "null plan");
    const ScaleLayout &L = *P->lay;
    if (L.kind == ScaleLayout::CHAIN) return L.chain_fused ? L.fast_hw : 0;
    return (L.kind == ScaleLayout::GENERIC || L.kind == ScaleLayout::GENERIC_UYVY) ? L.fast_hw : 0;
}

extern "C" int pp_scale_plan_stats(const pp_scale_plan *P, int64_t *out, int n) {
    if (!P || !out || n < 0) PP_FAIL(PP_ERR_INVALID, "null argument");
    const ScaleLayout &L = *P->lay;
    if (L.kind == ScaleLayout::COPY || L.kind == ScaleLayout::INTERLEAVE) return 0;
    const bool strip = L.fast_hw > 0;
    const PlaneJob &J = strip ? L.fjob[0] : L.job[0];
    const bool chain = L.kind == ScaleLayout::CHAIN && L.chain_fused;
    const int64_t v[] = {(int64_t)(chain ? L.chain_lds : strip ? L.fast_lds : L.lds_bytes),
                         strip ? L.fast_tw : pp::kThreads,
                         strip ? L.fast_tiles : L.job[2].tile_base + L.job[2].tiles_x * L.job[2].tiles_y, J.cho,
                         J.seg_h, J.vtp,
                         L.job[1].vtp, J.S, J.ring, J.maxnew};
    const int k = std::min<int>(n, (int)(sizeof(v) / sizeof(v[0])));
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

extern "C" int pp_scale_plan_filter(const pp_scale_plan *P, int which, int16_t *coef, int32_t *pos, int capacity) {
    if (!P || which < 0 || which > 3) PP_FAIL(PP_ERR_INVALID, "bad plan/which");
    const ScaleLayout &L = *P->lay;
    if (L.kind == ScaleLayout::COPY || L.kind == ScaleLayout::INTERLEAVE) return 0;
    const pp::FilterBank &f = L.f[which];
    if ((int64_t)f.n * f.size > capacity) PP_FAIL(PP_ERR_INVALID, "capacity %d < %d", capacity, f.n * f.size);
    std::memcpy(coef, f.coef.data(), f.coef.size() * 2);
    std::memcpy(pos, f.pos.data(), f.pos.size() * 4);
    return f.size;
}

namespace {

bool aligned(const void *p, int64_t ls, int64_t fs, int a) {
    return ((uintptr_t)p % a) == 0 && ls % a == 0 && fs % a == 0;
}

// every source plane pointer, linesize and (batches) frame stride 16-B aligned
bool vec_src(const pp_frames *src, int nframes) {
    bool v = true;
    for (int p = 0; p < 3; ++p) v &= aligned(src->data[p], src->linesize[p], nframes > 1 ? src->frame_stride[p] : 0, 16);
    return v;
}

// launch slot i reads plane sp of `src` and writes plane dp of `dst`
void set_plane(ScaleArgs &a, int i, const pp_frames *src, int sp, const pp_frames *dst, int dp) {
    a.src[i] = static_cast<const uint8_t *>(src->data[sp]);
    a.sls[i] = src->linesize[sp];
    a.sfs[i] = src->frame_stride[sp];
    a.dst[i] = static_cast<uint8_t *>(dst->data[dp]);
    a.dls[i] = dst->linesize[dp];
    a.dfs[i] = dst->frame_stride[dp];
}

// `k` over a.tiles workgroups per frame, as many frames per launch as the 1-D
// grid size limit allows
int launch_frames(KernelFn k, const ScaleArgs &a, int threads, size_t lds, int nframes, hipStream_t st) {
    const int fmax = std::max(1, (1 << 30) / a.tiles);
    for (int f0 = 0; f0 < nframes; f0 += fmax) {
        const int nf = std::min(fmax, nframes - f0);
        ScaleArgs b = a;
        for (int i = 0; i < a.nplanes; ++i) {
            b.src[i] += f0 * a.sfs[i];
            b.dst[i] += f0 * a.dfs[i];
        }
        hipLaunchKernelGGL(k, dim3(a.tiles * nf), dim3(threads), lds, st, b);
    }
    PP_HIP(hipGetLastError());
    return PP_OK;
}

// `tmp`: a planar batch at the plan's output size in the plan-owned scratch
// (one stream at a time), plane strides ys (luma) and cs (chroma) bytes
int scratch_batch(pp_scale_plan *P, int64_t ys, int64_t cs, int nframes, pp_frames *tmp) {
    if (P->scratch_frames < nframes) {
        if (P->scratch) PP_HIP(hipFree(P->scratch));
        P->scratch = nullptr;
        P->scratch_frames = 0;
        PP_HIP(hipMalloc(&P->scratch, (ys + 2 * cs) * nframes));
        P->scratch_frames = nframes;
    }
    uint8_t *s = static_cast<uint8_t *>(P->scratch);
    *tmp = pp_frames{};
    tmp->data[0] = s; tmp->data[1] = s + ys * nframes; tmp->data[2] = s + (ys + cs) * nframes;
    tmp->linesize[0] = P->lay->dw; tmp->linesize[1] = tmp->linesize[2] = P->lay->cdw;
    tmp->frame_stride[0] = ys; tmp->frame_stride[1] = tmp->frame_stride[2] = cs;
    return PP_OK;
}

// ---------------------------------------------------------------------------
// Which compiled kernel a launch runs.  The strip, packed, chain and general
// launchers below pick their kernel through these functions and
// pp_scale_plan_instances reports what they return, so for those launches the
// report is the choice.  Which launches a plan makes (plan_keys: unscaled
// converters, the two-launch chain, the scratch batch's alignment) restates
// execute_kind and has to be kept in step with it by hand.
struct KernelKey {
    int family;      // PP_SCALE_FAM_*
    int sbytes;      // source sample bytes
    int outb;        // output bits (a chain launch: the chain's target depth)
    int win;         // strip families: HW; general kernel: HT
    int vtm;         // strip families: V tap-pair bucket
    int direct;      // strip_kernel's DIRECT instance
    int tw256;       // 256-column strips
    int vtp2;        // second-stage V tap pairs (fuse-2 planes of a chain launch)
    int clamped;     // every strip of the launch takes the clamped V pass
    int clamp_path;  // the instance compiles the clamped V-pass copy
    int cho;         // output rows per chunk of the launch's first plane
    int chunks;      // fewest chunks a plane of the launch walks per segment (fuse-2 planes: over their height)
};

// chunk geometry of a launch over `np` jobs, for the report only
void key_chunks(KernelKey &k, const PlaneJob *const *jobs, int np) {
    k.cho = jobs[0]->cho;
    k.chunks = INT_MAX;
    for (int i = 0; i < np; ++i) {
        const PlaneJob &J = *jobs[i];
        const int rows = J.fuse == 2 ? J.dh : std::min(J.dh, J.seg_h);
        k.chunks = std::min(k.chunks, (rows + J.cho - 1) / J.cho);
    }
}

KernelFn kernel_for(const KernelKey &k) {
    using namespace pp;
    const bool u8 = k.sbytes == 1;
    switch (k.family) {
    case PP_SCALE_FAM_PLAIN:
        return u8 ? pick_strip_u8(k.outb, k.win, k.vtm, k.tw256 ? 256 : 512)
                  : pick_strip_u16(k.outb, k.win, k.vtm, k.tw256 ? 256 : 512);
    case PP_SCALE_FAM_PACKED: return u8 ? pick_strip_packed_u8(k.win, k.vtm) : pick_strip_packed_u16(k.win, k.vtm);
    case PP_SCALE_FAM_CHAIN:
        return u8 ? pick_strip_chain_u8(k.outb, k.win, k.vtm) : pick_strip_chain_u16(k.outb, k.win, k.vtm);
    case PP_SCALE_FAM_CHAIN_LUMA: return u8 ? pick_strip_luma_u8(k.win, k.vtm) : pick_strip_luma_u16(k.win, k.vtm);
    case PP_SCALE_FAM_CHAIN_CHROMA: return u8 ? pick_strip_chroma_u8(k.win, k.vtm) : pick_strip_chroma_u16(k.win, k.vtm);
    case PP_SCALE_FAM_GENERAL:
        if (u8) return k.outb == 8 ? pick_ht<uint8_t, 8>(k.win, k.tw256) : pick_ht<uint8_t, 10>(k.win, k.tw256);
        return k.outb == 8 ? pick_ht<uint16_t, 8>(k.win, k.tw256) : pick_ht<uint16_t, 10>(k.win, k.tw256);
    default: return nullptr;
    }
}

// a strip launch over `np` jobs is clamped when rows take vector stores and
// every plane's width is a multiple of 4 (strip.hpp: `clamp`, per strip)
bool jobs_clamped(const PlaneJob *const *jobs, int np, bool vdst) {
    bool c = vdst;
    for (int i = 0; i < np; ++i) c = c && (jobs[i]->dw & 3) == 0;
    return c;
}

// launch_generic: the strip kernel for strip plans on vector-loadable
// sources, else the general kernel's H-tap bucket
// (an 8-bit HW-8 plan takes the strip path only with its DIRECT tiling:
// that instance stages no rows)
KernelKey generic_key(const ScaleLayout &L, int out_depth, bool vsrc, bool vdst) {
    using namespace pp;
    KernelKey k{};
    k.sbytes = L.si.depth == 8 ? 1 : 2;
    k.outb = out_depth == 8 ? 8 : 10;
    if (L.fast_hw && vsrc && (L.direct || !(L.si.depth == 8 && L.fast_hw == 8))) {
        k.family = PP_SCALE_FAM_PLAIN;
        k.win = L.fast_hw;
        k.vtm = strip_vtm_bucket(std::max(L.fjob[0].vtp, L.fjob[1].vtp));
        k.direct = L.si.depth == 8 && L.fast_hw == 8;
        k.tw256 = L.fast_tw == 256;
        k.clamp_path = strip_clamp_rule(k.sbytes, k.outb, k.win, k.vtm, 0);
        const PlaneJob *jobs[3] = {&L.fjob[0], &L.fjob[1], &L.fjob[2]};
        k.clamped = k.clamp_path && jobs_clamped(jobs, 3, vdst);
        key_chunks(k, jobs, 3);
    } else {
        k.family = PP_SCALE_FAM_GENERAL;
        k.win = L.ht;
        k.tw256 = L.job[0].tw == kTileW && L.job[1].tw == kTileW && L.job[2].tw == kTileW;
        const PlaneJob *jobs[3] = {&L.job[0], &L.job[1], &L.job[2]};
        key_chunks(k, jobs, 3);
    }
    return k;
}

// launch_packed (never clamped: per-lane byte stores into the packed row)
KernelKey packed_key(const ScaleLayout &L) {
    KernelKey k{};
    k.family = PP_SCALE_FAM_PACKED;
    k.sbytes = L.si.depth == 8 ? 1 : 2;
    k.outb = 8;
    k.win = L.fast_hw;
    k.vtm = pp::strip_vtm_bucket(std::max(L.fjob[0].vtp, L.fjob[1].vtp));
    k.tw256 = 1;
    const PlaneJob *jobs[3] = {&L.fjob[0], &L.fjob[1], &L.fjob[2]};
    key_chunks(k, jobs, 3);
    return k;
}

// launch_chain_planes over `np` jobs with window `hw`
KernelKey chain_key(const ScaleLayout &L, bool has_luma, const PlaneJob *const *jobs, int np, int hw, bool luma_only,
                    bool vdst) {
    using namespace pp;
    KernelKey k{};
    k.sbytes = L.si.depth == 8 ? 1 : 2;
    k.outb = L.chain_out;
    k.win = hw;
    k.tw256 = 1;
    int vtp = 1;
    for (int i = 0; i < np; ++i) {
        vtp = std::max(vtp, jobs[i]->vtp);
        if (jobs[i]->fuse == 2) k.vtp2 = jobs[i]->vtp2;
    }
    k.vtm = strip_vtm_bucket(vtp);
    key_chunks(k, jobs, np);
    // the luma launch of a 10-bit chain (fuse 1 into 10 bits) takes its own
    // instance without the ring2 / second-stage code (FUSE 9)
    // (clamped plans only: every plane's width a multiple of 4 with vector
    // stores, so those instances compile the clamped V pass alone)
    const bool clamped = jobs_clamped(jobs, np, vdst);
    const bool l9 = clamped && luma_only && L.chain_out == 10 && jobs[0]->fuse == 1 && !PP_KNOB("PIXPATH_CHAIN_NO_LUMA9");
    // ... and the chroma launch (every plane fuse 2) FUSE 11
    bool c11 = clamped && !luma_only && has_luma && L.chain_out == 10 && !PP_KNOB("PIXPATH_CHAIN_NO_CHROMA11");
    for (int i = 0; i < np; ++i) c11 = c11 && jobs[i]->fuse == 2;
    if (l9 || c11) {  // (FUSE 9 / 11 exist for narrow windows only)
        k.family = l9 ? PP_SCALE_FAM_CHAIN_LUMA : PP_SCALE_FAM_CHAIN_CHROMA;
        k.clamp_path = k.clamped = 1;
        if (kernel_for(k)) return k;
    }
    k.family = PP_SCALE_FAM_CHAIN;
    k.clamp_path = strip_clamp_rule(k.sbytes, 8, k.win, k.vtm, L.chain_out);
    k.clamped = k.clamp_path && clamped;
    return k;
}

int launch_generic(pp_scale_plan *P, const pp_frames *src, const pp_frames *dst, int nframes, hipStream_t st,
                   int out_depth, bool allow_dither) {
    using namespace pp;
    const ScaleLayout &L = *P->lay;
    ScaleArgs a{};
    a.nplanes = 3;
    for (int p = 0; p < 3; ++p) {
        a.pl[p] = L.job[p];
        set_plane(a, p, src, p, dst, p);
    }
    a.hshift = L.si.depth == 8 ? 7 : L.si.depth - 1;
    a.dither = allow_dither && L.si.depth > 8 && out_depth == 8;
    a.vec_src = vec_src(src, nframes);
    a.vec_dst = 1;
    if (const char *e = PP_KNOB("PIXPATH_SCALE_DEBUG")) a.debug = atoi(e);
    for (int p = 0; p < 3; ++p)
        a.vec_dst &= aligned(a.dst[p], a.dls[p], nframes > 1 ? a.dfs[p] : 0, out_depth == 8 ? 4 : 8);
    size_t lds = L.lds_bytes;
    int threads = kThreads;
    a.tiles = L.job[2].tile_base + L.job[2].tiles_x * L.job[2].tiles_y;
    const KernelKey key = generic_key(L, out_depth, a.vec_src != 0, a.vec_dst != 0);
    if (key.family == PP_SCALE_FAM_PLAIN) {
        for (int p = 0; p < 3; ++p) a.pl[p] = L.fjob[p];
        lds = L.fast_lds;
        a.tiles = L.fast_tiles;
        threads = L.fast_tw;
    }
    KernelFn k = kernel_for(key);
    if (!k) PP_FAIL(PP_ERR_UNSUPPORTED, "no kernel for %d taps", L.ht);
    return launch_frames(k, a, threads, lds, nframes, st);
}

// GENERIC_UYVY on the strip path: one strip_kernel<.., FUSE = 1> launch whose
// planes store straight into the uyvy422 rows (U Y V Y byte order)
int launch_packed(pp_scale_plan *P, const pp_frames *src, const pp_frames *dst, int nframes, hipStream_t st) {
    using namespace pp;
    const ScaleLayout &L = *P->lay;
    ScaleArgs a{};
    a.nplanes = 3;
    static const int off[3] = {1, 0, 2}, step[3] = {2, 4, 4};
    for (int p = 0; p < 3; ++p) {
        a.pl[p] = L.fjob[p];
        a.pl[p].pk_off = off[p];
        a.pl[p].pk_step = step[p];
        set_plane(a, p, src, p, dst, 0);
    }
    a.hshift = L.si.depth == 8 ? 7 : L.si.depth - 1;
    a.dither = 0;  // yuv2packedX rounds with 1 << 18, never dithers
    a.vec_src = 1;
    a.vec_dst = 0;
    KernelFn k = kernel_for(packed_key(L));
    if (!k) PP_FAIL(PP_ERR_UNSUPPORTED, "no packed kernel for window %d", L.fast_hw);
    a.tiles = L.fast_tiles;
    return launch_frames(k, a, kThreads, L.fast_lds, nframes, st);
}

// CHAIN, fused: strip_kernel<.., FUSE = target depth> launches over the
// planes `pl` (job, source / destination plane index), tile bases renumbered
// for the launch
int launch_chain_planes(pp_scale_plan *P, const PlaneJob *const *jobs, const int *pl, int np, int hw, size_t lds,
                        const pp_frames *src, const pp_frames *dst, int nframes, hipStream_t st,
                        bool luma_only = false) {
    using namespace pp;
    const ScaleLayout &L = *P->lay;
    ScaleArgs a{};
    a.nplanes = np;
    for (int i = 0; i < np; ++i) {
        a.pl[i] = *jobs[i];
        a.pl[i].tile_base = a.tiles;
        a.tiles += a.pl[i].tiles_x * a.pl[i].tiles_y;
        set_plane(a, i, src, pl[i], dst, pl[i]);
    }
    a.hshift = L.si.depth == 8 ? 7 : L.si.depth - 1;
    a.dither = L.si.depth > 8;
    a.vec_src = 1;
    a.vec_dst = 1;
    if (const char *e = PP_KNOB("PIXPATH_SCALE_DEBUG")) a.debug = atoi(e);
    for (int i = 0; i < np; ++i)
        a.vec_dst &= aligned(a.dst[i], a.dls[i], nframes > 1 ? a.dfs[i] : 0, L.chain_out == 8 ? 4 : 8);
    KernelFn k = kernel_for(chain_key(L, P->luma != nullptr, jobs, np, hw, luma_only, a.vec_dst != 0));
    if (!k) PP_FAIL(PP_ERR_UNSUPPORTED, "no chain kernel for window %d", hw);
    return launch_frames(k, a, kThreads, lds, nframes, st);
}

// The launches of a fused CHAIN plan: one over all planes, or (P->luma) the
// luma launch of the plain first-stage plan, then the chroma planes' chain launch
struct ChainLaunch {
    const PlaneJob *jobs[3];
    int pl[3];
    int np, hw;
    size_t lds;
    bool luma_only;
};

int chain_launches(const pp_scale_plan *P, ChainLaunch out[2]) {
    const ScaleLayout &L = *P->lay;
    if (P->luma && P->luma->lay->fast_hw == L.fast_hw && PP_KNOB("PIXPATH_CHAIN_COMBINED")) {
        // measurement: the luma plan's job (32-row chunks) and the chroma
        // chain jobs in ONE launch, LDS the larger of the two layouts
        out[0] = ChainLaunch{{&P->luma->lay->fjob[0], &L.fjob[1], &L.fjob[2]}, {0, 1, 2}, 3, L.fast_hw,
                             std::max(P->luma->lay->fast_lds_plane[0], L.chain_lds), false};
        return 1;
    }
    if (P->luma) {
        const ScaleLayout &LL = *P->luma->lay;
        out[0] = ChainLaunch{{&LL.fjob[0], nullptr, nullptr}, {0, 0, 0}, 1, LL.fast_hw, LL.fast_lds_plane[0], true};
        out[1] = ChainLaunch{{&L.fjob[1], &L.fjob[2], nullptr}, {1, 2, 0}, 2, L.fast_hw, L.chain_lds, false};
        return 2;
    }
    out[0] = ChainLaunch{{&L.fjob[0], &L.fjob[1], &L.fjob[2]}, {0, 1, 2}, 3, L.fast_hw, L.chain_lds, false};
    return 1;
}

int launch_chain(pp_scale_plan *P, const pp_frames *src, const pp_frames *dst, int nframes, hipStream_t st) {
    using namespace pp;
    ChainLaunch cl[2];
    const int n = chain_launches(P, cl);
    auto go = [&](const ChainLaunch &c, hipStream_t s) {
        return launch_chain_planes(P, c.jobs, c.pl, c.np, c.hw, c.lds, src, dst, nframes, s, c.luma_only);
    };
    if (n == 1) return go(cl[0], st);
    // PIXPATH_CHAIN_OVERLAP (measurement build): the luma launch on a side
    // stream, concurrent with the chroma launch (fork / join events on `st`)
    const bool overlap = PP_KNOB("PIXPATH_CHAIN_OVERLAP") != nullptr;
    hipStream_t ls = st;
    if (overlap) {
        if (!P->side) {
            PP_HIP(hipStreamCreateWithFlags(&P->side, hipStreamNonBlocking));
            PP_HIP(hipEventCreateWithFlags(&P->fork, hipEventDisableTiming));
            PP_HIP(hipEventCreateWithFlags(&P->join, hipEventDisableTiming));
        }
        PP_HIP(hipEventRecord(P->fork, st));
        PP_HIP(hipStreamWaitEvent(P->side, P->fork, 0));
        ls = P->side;
    }
    if (int rc = go(cl[0], ls)) return rc;
    const int rc = go(cl[1], st);
    if (overlap) {
        PP_HIP(hipEventRecord(P->join, P->side));
        PP_HIP(hipStreamWaitEvent(st, P->join, 0));
    }
    return rc;
}

// which path a CHAIN / GENERIC_UYVY plan executes for a source alignment
bool chain_runs_fused(const ScaleLayout &L, bool vsrc) { return L.chain_fused && vsrc; }
bool packed_runs_strip(const ScaleLayout &L, bool vsrc) { return L.fast_hw && vsrc; }
// the plan-owned scratch batch (scratch_batch) has dense rows (linesize = plane
// width) in a fresh allocation: its alignment as a destination / source.
// Exact for the chain's scratch (frame strides rounded to 16 B); the packed
// path's strides are unrounded, so with more than one frame its general-kernel
// launch may store per lane where this says vector -- the same kernel either way.
bool scratch_aligned(const ScaleLayout &L, int a) { return L.dw % a == 0 && L.cdw % a == 0; }

// the keys of every launch execute_kind(P, kind, ...) makes
void plan_keys(const pp_scale_plan *P, ScaleLayout::Kind kind, bool vsrc, bool vdst, std::vector<KernelKey> &out) {
    const ScaleLayout &L = *P->lay;
    KernelKey k{};
    k.sbytes = L.si.depth == 8 ? 1 : 2;
    k.outb = L.di.depth == 8 ? 8 : 10;
    switch (kind) {
    case ScaleLayout::COPY:
        k.family = PP_SCALE_FAM_COPY;
        out.push_back(k);
        return;
    case ScaleLayout::INTERLEAVE:
        k.family = PP_SCALE_FAM_INTERLEAVE;
        out.push_back(k);
        return;
    case ScaleLayout::GENERIC:
        out.push_back(generic_key(L, L.di.depth, vsrc, vdst));
        return;
    case ScaleLayout::CHAIN: {
        if (chain_runs_fused(L, vsrc)) {
            ChainLaunch cl[2];
            const int n = chain_launches(P, cl);
            for (int i = 0; i < n; ++i)
                out.push_back(chain_key(L, P->luma != nullptr, cl[i].jobs, cl[i].np, cl[i].hw, cl[i].luma_only, vdst));
            return;
        }
        k.family = PP_SCALE_FAM_TWO_LAUNCH;
        k.outb = L.chain_out;
        out.push_back(k);
        plan_keys(P, L.first_kind, vsrc, scratch_aligned(L, 4), out);
        plan_keys(P->stage2, P->stage2->lay->kind, scratch_aligned(L, 16), vdst, out);
        return;
    }
    case ScaleLayout::GENERIC_UYVY:
        if (packed_runs_strip(L, vsrc)) {
            out.push_back(packed_key(L));
            return;
        }
        out.push_back(generic_key(L, 8, vsrc, scratch_aligned(L, 4)));
        k.family = PP_SCALE_FAM_INTERLEAVE;
        k.sbytes = 1;
        k.outb = 8;
        out.push_back(k);
        return;
    }
}

void launch_interleave(const pp_frames *src, const pp_frames *dst, int w, int h, int nframes, hipStream_t st) {
    dim3 grid(((w + 1) / 2 + 1023) / 1024, h, nframes);
    hipLaunchKernelGGL(pp::interleave_uyvy_kernel, grid, dim3(256), 0, st, (const uint8_t *)src->data[0],
                       (const uint8_t *)src->data[1], (const uint8_t *)src->data[2], src->linesize[0],
                       src->linesize[1], src->linesize[2], src->frame_stride[0], src->frame_stride[1],
                       src->frame_stride[2], (uint8_t *)dst->data[0], dst->linesize[0], dst->frame_stride[0], w, h);
}

}  // namespace

extern "C" int pp_scale_plan_instances(const pp_scale_plan *P, int vsrc, int vdst, int32_t *out, int capacity) {
    if (!P || !out || capacity < 0) PP_FAIL(PP_ERR_INVALID, "null argument");
    std::vector<KernelKey> keys;
    plan_keys(P, P->lay->kind, vsrc != 0, vdst != 0, keys);
    if ((int)keys.size() > capacity) PP_FAIL(PP_ERR_INVALID, "capacity %d < %d keys", capacity, (int)keys.size());
    for (size_t i = 0; i < keys.size(); ++i) {
        const KernelKey &k = keys[i];
        const int32_t v[PP_SCALE_KEY_FIELDS] = {k.family, k.sbytes, k.outb,    k.win,        k.vtm, k.direct,
                                                k.tw256,  k.vtp2,   k.clamped, k.clamp_path, k.cho, k.chunks};
        std::memcpy(out + i * PP_SCALE_KEY_FIELDS, v, sizeof(v));
    }
    return (int)keys.size();
}

static int execute_kind(pp_scale_plan *P, ScaleLayout::Kind kind, const pp_frames *src, const pp_frames *dst,
                        int nframes, void *stream) {
    using namespace pp;
    const ScaleLayout &L = *P->lay;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t yb = (int64_t)L.dw * L.dh, cb = (int64_t)L.cdw * L.cdh;
    switch (kind) {
    case ScaleLayout::COPY: {
        const int sbytes = L.si.depth > 8 ? 2 : 1, dbytes = L.di.depth > 8 ? 2 : 1;
        for (int p = 0; p < 3; ++p) {
            const int w = p ? L.csw : L.sw, h = p ? L.csh : L.sh;
            dim3 grid((w + 2047) / 2048, h, nframes);
            hipLaunchKernelGGL(copy_widen_kernel, grid, dim3(256), 0, st, (const uint8_t *)src->data[p],
                               src->linesize[p], src->frame_stride[p], sbytes, (uint8_t *)dst->data[p],
                               dst->linesize[p], dst->frame_stride[p], dbytes, w, h, L.di.depth - L.si.depth);
        }
        PP_HIP(hipGetLastError());
        return PP_OK;
    }
    case ScaleLayout::INTERLEAVE:
        launch_interleave(src, dst, L.sw, L.sh, nframes, st);
        PP_HIP(hipGetLastError());
        return PP_OK;
    case ScaleLayout::GENERIC:
        return launch_generic(P, src, dst, nframes, st, L.di.depth, true);
    case ScaleLayout::CHAIN: {
        if (chain_runs_fused(L, vec_src(src, nframes))) return launch_chain(P, src, dst, nframes, st);
        // two launches through a yuv420p scratch batch
        pp_frames tmp;
        if (int rc = scratch_batch(P, (yb + 15) & ~int64_t(15), (cb + 15) & ~int64_t(15), nframes, &tmp)) return rc;
        if (int rc = execute_kind(P, L.first_kind, src, &tmp, nframes, stream)) return rc;
        return pp_scale_execute(P->stage2, &tmp, dst, nframes, stream);
    }
    case ScaleLayout::GENERIC_UYVY: {
        if (packed_runs_strip(L, vec_src(src, nframes))) return launch_packed(P, src, dst, nframes, st);
        // yuv2packedX: planar 8-bit 4:2:2 (flat rounding: 1 << 18, never dithers) then interleave
        pp_frames tmp;
        if (int rc = scratch_batch(P, yb, cb, nframes, &tmp)) return rc;
        if (int rc = launch_generic(P, src, &tmp, nframes, st, 8, false)) return rc;
        launch_interleave(&tmp, dst, L.dw, L.dh, nframes, st);
        PP_HIP(hipGetLastError());
        return PP_OK;
    }
    }
    PP_FAIL(PP_ERR_INVALID, "bad plan kind");
}

extern "C" int pp_scale_execute(pp_scale_plan *P, const pp_frames *src, const pp_frames *dst, int nframes,
                                void *stream) {
    if (!P || !src || !dst || nframes < 0) PP_FAIL(PP_ERR_INVALID, "null argument");
    if (!P->ctx) PP_FAIL(PP_ERR_INVALID, "host-only plan (created without a context) cannot execute");
    if (nframes == 0) return PP_OK;
    PP_HIP(hipSetDevice(P->ctx->device));
    return execute_kind(P, P->lay->kind, src, dst, nframes, stream);
}

