// Host side of the skeleton the analysis kernels share: the geometry of a plane
// and the checks of a pp_frames against it (pp_metrics, pp_frame_adler32,
// pp_frame_stats); the same for the bare luma planes of pp_frame_sse_band,
// pp_ms_ssim, pp_vif, pp_adm, pp_motion and pp_banding, with their frame map
// and the frames one launch takes; and the scratch buffers the context keeps
// for partials and workspaces.  Device side: analysis_dev.hpp.
#pragma once

#include <algorithm>

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

// The planes of a luma-only entry point: w x h samples of `bitdepth` bits, each
// given as pointer, pitch and frame stride.  luma_open, one luma_plane per plane,
// luma_close, in that order: it is the order the failures are reported in.
struct LumaPlanes {
    int es = 1;           // bytes of a sample
    PlaneGeom g{};
    bool aligned = true;  // every plane so far lies on the 16-B grid (check_plane)
    uint64_t bits = 0;    // the or of every pointer, pitch and frame stride so far
};

inline int luma_open(LumaPlanes &lp, int bitdepth, int w, int h) {
    if (bitdepth != 8 && bitdepth != 10) PP_FAIL(PP_ERR_INVALID, "bitdepth %d (8 or 10)", bitdepth);
    if (w < 1 || h < 1) PP_FAIL(PP_ERR_INVALID, "frame %dx%d", w, h);
    lp.es = bitdepth > 8 ? 2 : 1;
    lp.g.pw = w; lp.g.ph = h; lp.g.rb = (int64_t)w * lp.es;
    return PP_OK;
}

// check_plane of one plane (`single`: one frame, its stride is not looked at).
inline int luma_plane(LumaPlanes &lp, const void *data, int64_t ls, int64_t fs, const char *who, int halo_rows = 0,
                      bool single = false) {
    pp_frames fr{};
    fr.data[0] = const_cast<void *>(data); fr.linesize[0] = ls; fr.frame_stride[0] = single ? 0 : fs;
    lp.bits |= (uintptr_t)data | (uint64_t)ls | (uint64_t)fr.frame_stride[0];
    return check_plane(&fr, 0, lp.g, lp.aligned, halo_rows, who, single);
}

inline int luma_close(const LumaPlanes &lp) {
    if (lp.bits & (uint64_t)(lp.es - 1)) PP_FAIL(PP_ERR_INVALID, "16-bit samples off the 2-byte grid");
    return PP_OK;
}

// The words of a frame map's two messages: shown frame k of n reads frame
// map[k] (k without a map) of a pool of npool.
struct MapNames {
    const char *map, *n, *npool, *kind;
};
constexpr MapNames kRefIndexMap{"ref_index", "ndist", "nref", "reference"};
constexpr MapNames kIndexMap{"index", "n", "nsrc", "source"};

inline int check_frame_map(const int32_t *map, int n, int npool, const MapNames &nm) {
    if (map) {
        for (int k = 0; k < n; ++k)
            if (map[k] < 0 || map[k] >= npool)
                PP_FAIL(PP_ERR_INVALID, "%s[%d] = %d outside the %d %s frames", nm.map, k, map[k], npool, nm.kind);
    } else if (n > npool) {
        PP_FAIL(PP_ERR_INVALID, "%s %d > %s %d without %s", nm.n, n, nm.npool, npool, nm.map);
    }
    return PP_OK;
}

// A frame map travels in the kernel arguments, kFrameMap entries per launch;
// launches on one stream run in order, so they share the context's workspace.
constexpr int kFrameMap = 256;
constexpr int64_t kLaunchWork = 1 << 30;  // bytes of workspace a launch may hold (at least one frame's)

// Frames of n one launch takes: the map's room, and a workspace within `budget`.
inline int frames_per_launch(int n, int64_t bytes_per_frame = 0, int64_t budget = kLaunchWork) {
    const int64_t fit = std::max<int64_t>(1, budget / std::max<int64_t>(bytes_per_frame, 1));
    return (int)std::min<int64_t>(std::min(n, kFrameMap), fit);
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
