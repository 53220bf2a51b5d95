// Geometry and path predicates of the unpack kernel (unpack.hip), shared by
// the kernel and its host launch code (pp_unpack_execute): the host's checked
// geometry and the kernel's per-row, per-chunk and per-piece choices are the
// same constexpr functions, as pack_plan.hpp's are for the packers.
//
// Terms.  A chunk is one 16-B input granule: 6 pixels of v210 (12 samples:
// U0 Y0 V0 | Y1 U1 Y2 | V1 Y3 U2 | Y4 V2 Y5, three 10-bit fields a word) or
// 8 pixels of uyvy422 (U Y0 V Y1 a word).  A piece is one 16-B output granule
// of a planar row: 8 samples at 10 bits, 16 at 8.  A workgroup (one wave) owns
// one output row of one frame: it decodes the chunks that overlap the window
// into an LDS row [Y | U | V] and then writes the row out piece by piece.
#pragma once

#include <cstddef>
#include <cstdint>

#include "pack_plan.hpp"

namespace pp {

constexpr int kUnpackLanes = 64;    // one wave per output row (as cpvs.hip)
constexpr int kUnpackUnroll = 4;    // 16-B chunk loads a lane keeps in flight
constexpr int kUnpackPass = kUnpackLanes * kUnpackUnroll;  // chunks decoded per trip of the row loop
constexpr size_t kUnpackLdsMax = 64 * 1024;

PP_HD constexpr int unpack_px(bool v210) { return v210 ? 6 : 8; }  // pixels per input chunk
PP_HD constexpr int unpack_es(bool v210) { return v210 ? 2 : 1; }  // output sample bytes
// bytes of a line that hold samples: whole 16-B groups of v210 (v210dec reads words), 2 W of uyvy422
PP_HD constexpr int64_t unpack_line_bytes(int W, bool v210) { return v210 ? (int64_t)((W + 5) / 6) * 16 : 2LL * W; }
// chunks [first, last] overlap the window's pixels [x, x + w)
PP_HD constexpr int unpack_first_chunk(int x, bool v210) { return x / unpack_px(v210); }
PP_HD constexpr int unpack_last_chunk(int x, int w, bool v210) { return (x + w - 1) / unpack_px(v210); }
// LDS row: luma and each chroma plane padded to whole pieces (cpvs_lds_stride)
PP_HD constexpr int unpack_pieces(int n, int es) { return (int)(((int64_t)n * es + 15) / 16); }
PP_HD constexpr size_t unpack_lds_bytes(int w, int cw, int es) {
    return (size_t)(unpack_pieces(w, es) + 2 * unpack_pieces(cw, es)) * 16;
}

// ---- per launch ---------------------------------------------------------------
// 16-B chunk loads: every indexable source row starts on the 16-B grid
PP_HD constexpr bool unpack_src_vec(uintptr_t addr, int64_t ls, int64_t fs, int frames) {
    return plane_aligned(addr, ls, fs, frames);
}
// 16-B piece stores of one destination plane
PP_HD constexpr bool unpack_dst_vec(uintptr_t addr, int64_t ls, int64_t fs, int frames) {
    return plane_aligned(addr, ls, fs, frames);
}
// the window starts on a whole chunk: its samples land in LDS as whole words
PP_HD constexpr bool unpack_grid(int x, bool v210) { return x % unpack_px(v210) == 0; }

// ---- per chunk ------------------------------------------------------------------
// chunk q goes to LDS with vector writes: window on the chunk grid and every
// pixel of the chunk inside the window (so inside the line: x + w <= W).
// Otherwise sample by sample, each sample tested against the window: a window
// at pixel phase 2 or 4 of a v210 group, the ragged last chunk, the W % 6 tails.
PP_HD constexpr bool unpack_chunk_vec(bool grid, int q, int x, int w, bool v210) {
    return grid && q * unpack_px(v210) >= x && (q + 1) * unpack_px(v210) <= x + w;
}
// sample of the window at luma column s / chroma column c
PP_HD constexpr bool unpack_sample_in(int s, int n) { return s >= 0 && s < n; }
// byte b of a line is read on the sample-by-sample load path
PP_HD constexpr bool unpack_byte_in(int64_t b, int64_t line_bytes) { return b < line_bytes; }

// ---- per piece ------------------------------------------------------------------
// samples of piece j that lie inside a row of n samples
PP_HD constexpr int unpack_piece_valid(int j, int n, int es) {
    return n - j * (16 / es) < 16 / es ? n - j * (16 / es) : 16 / es;
}
// one 16-B store, or the valid samples one by one (unaligned plane, ragged last piece)
PP_HD constexpr bool unpack_piece_vec(bool dvec, int valid, int es) { return dvec && valid == 16 / es; }

// Checked geometry of a launch: what pp_unpack_execute computes before it
// launches, and the error it returns for a launch it rejects.
struct UnpackGeom {
    bool v210, luma_only, empty;
    int W, H, x, y, w, h, cw, es;
    int q0, nq;          // first chunk and chunk count of the window
    int ny, nc;          // pieces of a luma / chroma row
    int src_vec, grid;
    int dst_vec[3];
    size_t lds;
};
int unpack_geometry(int in_fmt, int W, int H, const pp_frames *src, int x, int y, int w, int h, const pp_frames *dst,
                    int nframes, UnpackGeom *g);

}  // namespace pp
