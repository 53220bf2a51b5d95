// Host side of the skeleton the analysis reducers share (pp_metrics,
// pp_frame_adler32, pp_frame_stats): the geometry of a plane, the checks of a
// pp_frames against it, and the scratch buffers the context keeps for their
// partials.  Device side: analysis_dev.hpp.
#pragma once

#include "common.hpp"
#include "device.hpp"
#include "pack_plan.hpp"

namespace pp {

struct PlaneGeom {
    int pw, ph;      // samples of a row (pixels of a packed one); rows
    int64_t rb;      // bytes of a row that count
    int64_t ls, fs;  // of the pp_frames check_plane saw last
};

// Plane p of a w x h frame.  A packed format has plane 0 alone, its rows the
// packets' (v210: 128 bytes per 48 pixels; uyvy422: 2 bytes a pixel).
inline PlaneGeom plane_geom(int fmt, int w, int h, int p) {
    const FmtInfo fi = fmt_info(fmt);
    PlaneGeom g{};
    g.pw = p ? ceil_rshift(w, fi.hsub) : w;
    g.ph = p ? ceil_rshift(h, fi.vsub) : h;
    g.rb = fmt == PP_FMT_V210 ? v210_linesize(w) : fmt == PP_FMT_UYVY422 ? 2LL * w : (int64_t)g.pw * (fi.depth > 8 ? 2 : 1);
    return g;
}

// Plane p of `fr` against g: data present, the pitch holds a row, the lane
// offsets of rows 0 .. ph + halo_rows - 1 inside the 31-bit buffer range.
// Leaves pitch and frame stride in g; clears `aligned` unless pointer, pitch and
// frame stride (`single`: one frame, no stride) lie on the 16-B grid.  `who`
// prefixes the messages; `merged`: pp_metrics' one message for null and short.
inline int check_plane(const pp_frames *fr, int p, PlaneGeom &g, bool &aligned, int halo_rows = 0, const char *who = "",
                       bool single = false, bool merged = false) {
    const int64_t ls = g.ls = fr->linesize[p], fs = g.fs = fr->frame_stride[p];
    if (merged) {
        if (!fr->data[p] || ls < g.rb) PP_FAIL(PP_ERR_INVALID, "%splane %d: null data or short linesize", who, p);
    } else {
        if (!fr->data[p]) PP_FAIL(PP_ERR_INVALID, "%splane %d: null data", who, p);
        if (ls < g.rb)
            PP_FAIL(PP_ERR_INVALID, "%splane %d: linesize %lld below the row's %lld bytes", who, p, (long long)ls, (long long)g.rb);
    }
    if ((int64_t)(g.ph + halo_rows) * ls >= (int64_t)kOobOff)
        PP_FAIL(PP_ERR_UNSUPPORTED, "plane %d of %lld bytes exceeds the 2 GiB buffer range", p, (long long)(g.ph * ls));
    aligned &= !(((uintptr_t)fr->data[p] | (uint64_t)ls | (single ? 0 : (uint64_t)fs)) & 15);
    return PP_OK;
}

// Grown on demand, kept by the context (hipFree waits for earlier users).
inline int grow(Scratch &s, size_t need) {
    if (need <= s.cap) return PP_OK;
    if (s.buf) PP_HIP(hipFree(s.buf));
    s.buf = nullptr; s.cap = 0;
    PP_HIP(hipMalloc(&s.buf, need));
    s.cap = need;
    return PP_OK;
}

}  // namespace pp
