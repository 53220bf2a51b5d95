// Geometry and arm predicates of the pad / stall row kernels (pack.hip) and
// the fused CPVS kernel (cpvs.hip), shared by the kernels, their host launch
// code and the host-only arm walker (pack_plan.cpp, pp_pack_arms).
//
// Every condition that selects a code path of those kernels -- per launch,
// per row, per 16-B chunk, per chroma group -- is one constexpr function
// here.  The kernels call them instead of spelling the condition, and the
// walker calls the same functions over the same rows / chunks / groups, so
// the set of arms it reports is what the launch executes, not a second
// statement of it.  The arms are named by enum pp_pack_arm (include/pixpath.h).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "common.hpp"

#if defined(PIXPATH_HOST_ONLY) || !defined(__HIPCC__)
#define PP_HD
#else
#define PP_HD __host__ __device__
#endif

namespace pp {

// ---- shared ----------------------------------------------------------------
// vf_pad offsets: v < 0 is the centring expression (outer - inner) / 2,
// truncated; then ff_draw_round_to_sub(.., -1, ..): down to the chroma grid.
// The stall's centred spinner origin is the same rule (it may be negative).
PP_HD constexpr int pad_offset(int v, int outer, int inner, int sub) {
    return ((v < 0 ? (outer - inner) / 2 : v) >> sub) << sub;
}
PP_HD constexpr bool pad_exceeds(int off, int inner, int outer) { return off + inner > outer; }
// rows [off, off + n) of the output are the input's
PP_HD constexpr bool row_live(int iy, int n) { return iy >= 0 && iy < n; }
// a plane of `frames` indexable frames is 16-B aligned at every row start
PP_HD constexpr bool plane_aligned(uintptr_t addr, int64_t ls, int64_t fs, int frames) {
    return !(addr & 15) && !(ls & 15) && (frames < 2 || !(fs & 15));
}
PP_HD constexpr int64_t v210_linesize(int w) { return (int64_t)((w + 47) / 48) * 48 * 8 / 3; }

// ---- fused CPVS kernel -------------------------------------------------------
constexpr int kCpvsLanes = 64;   // one wave per canvas row (4-wave rows: 2.05 vs 1.64 ms, v210 1080p)
constexpr int kCpvsTaps = 4;     // bicubic 2x chroma: at most 4 rows per output row
constexpr int kStageUnroll = 8;  // 16-B staging loads a lane keeps in flight
constexpr int kCpvsStagePass = kCpvsLanes * kStageUnroll;  // 16-B pieces staged per pass
constexpr size_t kCpvsLdsMax = 64 * 1024;

// LDS row stride: n samples of es bytes rounded up to whole 16-B groups
PP_HD constexpr int cpvs_lds_stride(int n, int es) { return (int)(((int64_t)n * es + 15) / 16 * 16 / es); }
PP_HD constexpr size_t cpvs_lds_bytes(int ys, int cs, int es) { return (size_t)(ys + 2 * cs) * es; }
PP_HD constexpr int cpvs_px(int depth) { return depth == 8 ? 8 : 6; }  // pixels per 16-B output chunk
PP_HD constexpr int cpvs_chunks(int W, bool v210) { return v210 ? (int)(v210_linesize(W) / 16) : (W + 7) / 8; }
// 16-B pieces of the staged row: luma, and each chroma plane (4:2:0 chroma is filtered, not staged)
PP_HD constexpr int cpvs_stage_luma(int ys, int es) { return ys * es / 16; }
PP_HD constexpr int cpvs_stage_chroma(int cs, int es, bool v420) { return v420 ? 0 : cs * es / 16; }
// vertical tap k of a 4:2:0 output row reads AVPVS chroma row r, or black outside
PP_HD constexpr bool cpvs_tap_in(int k, int vt, int r, int ch) { return k < vt && r >= 0 && r < ch; }
PP_HD constexpr int cpvs_groups(int cw) { return (cw + 7) / 8; }  // 8-sample chroma groups
// A chroma group of a tap row loads as one vector when the rows are 16-B
// aligned.  No group of such a row lies past its padded end: cs is cw rounded
// up to a whole 16-B group (16 samples at 8 bits, 8 at 10), so
// cs / 8 >= ceil(cw / 8) = cpvs_groups(cw) for every cw (checked over a range
// of widths by tests/test_pack_arms.py); the kernel's former `g < cs / 8` term
// was always true and is gone.
PP_HD constexpr bool cpvs_group_vec(int aligned) { return aligned != 0; }
// sample e of group g on the sample-by-sample path: the ragged last group repeats the last sample
PP_HD constexpr bool cpvs_group_clamped(int g, int cw) { return g * 8 + 7 > cw - 1; }
PP_HD constexpr int cpvs_group_sample(int g, int e, int cw) { return g * 8 + e < cw - 1 ? g * 8 + e : cw - 1; }
// 8-bit: a chunk wholly inside the AVPVS with the pad offset on an 8-px grid
// reads its 8 Y and 4 + 4 chroma samples as 3 LDS words
PP_HD constexpr bool cpvs_fast8(int depth, int ox) { return depth == 8 && (ox & 7) == 0; }
PP_HD constexpr bool cpvs_fast8_chunk(bool fast8, bool live, int x0, int ox, int w, int cw, int W) {
    return fast8 && live && x0 - ox >= 0 && x0 - ox + 8 <= w && x0 / 2 - (ox >> 1) + 4 <= cw && x0 + 8 <= W;
}
PP_HD constexpr bool uyvy_chunk_full(int x0, int W) { return x0 + 8 <= W; }
// v210 chunk q of a line of (even) W pixels: six whole pixels, the encoder's
// tail of 2 or 4 pixels, or the zero fill up to the line size
enum V210Chunk { kV210Full, kV210Tail2, kV210Tail4, kV210Zero };
PP_HD constexpr int v210_chunk(int q, int W) {
    return q < W / 6 ? kV210Full : (q > W / 6 || W % 6 < 2) ? kV210Zero : (W % 6 < 4 ? kV210Tail2 : kV210Tail4);
}

// ---- row kernels (pad, stall) ---------------------------------------------------
constexpr int kRowLanes = 64;  // one wave per row
constexpr int kRowUnroll = 4;  // 16-B chunks a lane keeps in flight
constexpr int kRowPass = kRowLanes * kRowUnroll;
constexpr int kStallLaunchFrames = 256;  // output frames per stall launch (their indices are kernel arguments)

PP_HD constexpr int row_chunks(int W, int n) { return (W + n - 1) / n; }
// vector source loads: every indexable source row 16-B aligned and the shift a whole number of chunks
PP_HD constexpr bool row_src_vec(uintptr_t addr, int64_t ls, int64_t fs, int frames, int ox, int es) {
    return plane_aligned(addr, ls, fs, frames) && !((ox * es) & 15);
}
PP_HD constexpr bool row_dst_vec(uintptr_t addr, int64_t ls, int64_t fs, int frames) {
    return plane_aligned(addr, ls, fs, frames);
}
// the n source samples of a chunk at source column sx: one 16-B load, or sample by sample
PP_HD constexpr bool chunk_src_vec(bool row, bool vec, int sx, int n, int iw) {
    return row && vec && sx >= 0 && sx + n <= iw;
}
PP_HD constexpr bool chunk_src_outside(int sx, int n, int iw) { return sx + n <= 0 || sx >= iw; }
PP_HD constexpr bool chunk_dst_vec(bool dvec, int x, int n, int W) { return dvec && x + n <= W; }
PP_HD constexpr bool chunk_sample_stored(int x, int W) { return x < W; }
// stall: the chunk [x, x + n) of a spinner row touches the spinner's columns [px0, px0 + pw)
PP_HD constexpr bool stall_chunk_blends(bool in_rows, int x, int n, int px0, int pw) {
    return in_rows && x + n > px0 && x < px0 + pw;
}
PP_HD constexpr bool stall_sample_blends(int sx, int pw) { return sx >= 0 && sx < pw; }

// Per-plane geometry of a row kernel launch.
struct RowPlane {
    const uint8_t *src;
    int64_t sls, sfs;
    uint8_t *dst;
    int64_t dls, dfs;
    int W, rows;       // output plane width (samples) and rows
    int iw, ih;        // source plane size
    int ox, oy;        // source offset on the output plane (pad); 0 for stall
    int black;
    int vec;           // row_src_vec: vector loads
    int dvec;          // row_dst_vec: vector stores
};

// ---- host side ---------------------------------------------------------------
// row-kernel plane geometry from the C-ABI frame descriptors; sframes / dframes:
// the source and destination frames the launch can index
void row_planes(RowPlane *pl, const FmtInfo &fi, const pp_frames *src, const pp_frames *dst, int sframes, int dframes,
                int sw, int sh, int dw, int dh, int x, int y);

// Checked geometry of the three operations: what pp_pad_execute,
// pp_cpvs_execute and pp_stall_compose compute before they launch, and the
// error (code and message) each returns for a launch it rejects.  `empty`:
// nothing to launch (nframes == 0).
struct PadGeom {
    FmtInfo fi;
    RowPlane pl[3];
    int nframes;
    bool empty;
};
int pad_geometry(int fmt, int sw, int sh, const pp_frames *src, int dw, int dh, int x, int y, const pp_frames *dst,
                 int nframes, PadGeom *g);

struct CpvsGeom {
    FmtInfo fi;
    int w, h, cw, ch, W, H, ox, oy;
    int chunks, ys, cs, aligned, es;
    bool v210, v420, empty;
    size_t lds;
    int nframes;
};
int cpvs_geometry(int src_fmt, int w, int h, const pp_frames *src, int W, int H, int x, int y, int out_fmt,
                  const pp_frames *dst, int nframes, CpvsGeom *g);
// Bicubic 4:2:0 -> 4:2:2 chroma rows of the CLI's auto-inserted converter
// (sws_init_context with chrSrcH = ceil(H/2), chrDstH = H, centred siting),
// compacted: first padded-chroma row per output row and vt coefficients each.
int cpvs_vfilter(int H, int *vt, std::vector<int32_t> *pos, std::vector<int16_t> *coef);

#ifndef PIXPATH_STALL_G
#define PIXPATH_STALL_G 6
#endif
struct StallGeom {
    FmtInfo fi;
    RowPlane pl[3];
    int sw, sh, ox, oy;  // spinner size (0: none used) and origin, luma
    int nframes, G;
    bool empty;
};
int stall_geometry(int fmt, int w, int h, const pp_frames *src, const int32_t *src_index, const int32_t *spinner_index,
                   const pp_frames *dst, int nframes, int spin_fmt, int spin_n, int spin_w, int spin_h, StallGeom *g);

}  // namespace pp
