// Host side of the skeleton the analysis kernels share (device side:
// analysis_dev.hpp).  An entry point calls these pieces in this order, which is
// the order a call's faults are reported in ("Analysis skeleton"):
//   checks     planar pair: format, size, counts, check_pair, check_frame_map;
//              luma pair and shown sequence: luma_checks; an entry with a check
//              of its own in between calls luma_open, luma_plane, luma_close,
//              check_frame_map itself; one clip: plane_geom, check_plane
//   nothing    `if (n == 0) return PP_OK;` before any HIP call
//   arguments  put_pair / put_luma_pair, then the tiling of its own
//   scratch    frames_per_launch, grow of its own buffer of the context
//   instance   PP_PICK / PP_PICK_EDGE
//   launches   each_launch, fill_map, put_shown_before, the launches of its own
#pragma once

#include <algorithm>
#include <type_traits>

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

// Two planar clips as check_pair leaves them: checked, with their planes' geometry.
struct PairPlanes {
    const pp_frames *ref, *dist;
    PlaneGeom g[3];
    bool aligned = true;  // every plane of both lies on the 16-B grid
};

// check_plane of `ref`, then `dist`, plane by plane, each followed by its own
// test of the 2-byte grid.  halo_rows, the prefixes and `merged` as check_plane's.
inline int check_pair(PairPlanes &pl, int fmt, int w, int h, const pp_frames *ref, const pp_frames *dist,
                      int halo_rows = 0, const char *ref_who = "ref ", const char *dist_who = "dist ", bool merged = false) {
    const int es = fmt_info(fmt).depth > 8 ? 2 : 1;
    pl.ref = ref; pl.dist = dist;
    const pp_frames *both[2] = {ref, dist};
    const char *who[2] = {ref_who, dist_who};
    for (int p = 0; p < 3; ++p) {
        PlaneGeom &g = pl.g[p] = plane_geom(fmt, w, h, p);
        for (int c = 0; c < 2; ++c) {
            if (int e = check_plane(both[c], p, g, pl.aligned, halo_rows, who[c], false, merged)) return e;
            if (((uintptr_t)both[c]->data[p] | (uint64_t)g.ls | (uint64_t)g.fs) & (es - 1))
                PP_FAIL(PP_ERR_INVALID, "%splane %d: 16-bit samples off the 2-byte grid", who[c], p);
        }
    }
    return PP_OK;
}

// Into the members of MetArgs, CieArgs, HvsArgs.
template <typename Args>
inline void put_pair(Args &a, const PairPlanes &pl) {
    for (int p = 0; p < 3; ++p) {
        a.ref[p] = static_cast<const uint8_t *>(pl.ref->data[p]);
        a.dist[p] = static_cast<const uint8_t *>(pl.dist->data[p]);
        a.rls[p] = pl.ref->linesize[p]; a.rfs[p] = pl.ref->frame_stride[p];
        a.dls[p] = pl.dist->linesize[p]; a.dfs[p] = pl.dist->frame_stride[p];
    }
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

// The words of a luma family's messages: shown frame k of n reads frame map[k]
// (k without a map) of a pool of npool; the prefixes of the pool's plane and of
// the second plane, which holds the n shown frames or the one shown before them.
struct MapNames {
    const char *map, *n, *npool, *kind, *pool, *other;
};
constexpr MapNames kRefIndexMap{"ref_index", "ndist", "nref", "reference", "ref ", "dist "};
constexpr MapNames kIndexMap{"index", "n", "nsrc", "source", "src ", "prev "};

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

// n frames of bare luma planes, as an entry point is handed them.
struct LumaClip {
    const void *data;
    int64_t ls, fs;
    int n;
};

// The checks of the luma pair (kRefIndexMap: `other` the n = ndist frames) and the shown
// sequence (kIndexMap: `other` the `single` frame shown before, or none) up to the
// `n == 0` that is the caller's; pp_banding and pp_frame_sse_band call the pieces.
inline int luma_checks(LumaPlanes &lp, int bitdepth, int w, int h, const LumaClip &pool, const LumaClip &other, bool single,
                       const int32_t *map, int n, const MapNames &nm) {
    if (int e = luma_open(lp, bitdepth, w, h)) return e;
    if (n < 0) PP_FAIL(PP_ERR_INVALID, "%s %d < 0", nm.n, n);
    if (pool.n < 0) PP_FAIL(PP_ERR_INVALID, "%s %d < 0", nm.npool, pool.n);
    if (int e = luma_plane(lp, pool.data, pool.ls, pool.fs, nm.pool)) return e;
    if (other.data)
        if (int e = luma_plane(lp, other.data, other.ls, other.fs, nm.other, 0, single)) return e;
    if (int e = luma_close(lp)) return e;
    return check_frame_map(map, n, pool.n, nm);
}

// Into the members of MsArgs, VifArgs, AdmArgs, AlnArgs.
template <typename Args>
inline void put_luma_pair(Args &a, const LumaClip &ref, const LumaClip &dist) {
    a.ref = static_cast<const uint8_t *>(ref.data);
    a.dist = static_cast<const uint8_t *>(dist.data);
    a.rls = ref.ls; a.rfs = ref.fs;
    a.dls = dist.ls; a.dfs = dist.fs;
}

// Into b.prev / b.pls the frame shown before the first of the launch at k0: the
// sequence's, else `prev`, else none: the first stands in and what it gives is never
// reported.  Returns first_absent.  b.src, b.ls, b.fs and b.idx are filled.
template <typename Args>
inline int put_shown_before(Args &b, const int32_t *index, int k0, const void *prev, int64_t prev_linesize) {
    b.prev = b.src + (int64_t)(k0 > 0 ? (index ? index[k0 - 1] : k0 - 1) : b.idx[0]) * b.fs;
    b.pls = b.ls;
    if (k0 == 0 && prev) { b.prev = static_cast<const uint8_t *>(prev); b.pls = prev_linesize; }
    return k0 == 0 && !prev;
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

// body(k0, nk) per launch of n frames, `per` at a time; a code it returns ends the walk.
template <typename Body>
inline int each_launch(int n, int per, Body body) {
    for (int k0 = 0; k0 < n; k0 += per) {
        const int nk = std::min(per, n - k0);
        if constexpr (std::is_void_v<decltype(body(k0, nk))>) body(k0, nk);
        else if (int e = body(k0, nk)) return e;
    }
    return PP_OK;
}

// The launch's entries of a frame map: map[k0 ..], or the identity there.
inline void fill_map(int32_t *idx, const int32_t *map, int k0, int nk) {
    for (int k = 0; k < nk; ++k) idx[k] = map ? map[k0 + k] : k0 + k;
}

// The instance of K<S, ALIGNED> or K<S, ALIGNED, RAGGED> for sample type (or size) S;
// off the 16-B grid everything goes element by element, the ragged instance.
#define PP_PICK(K, S, aligned) ((aligned) ? K<S, true> : K<S, false>)
#define PP_PICK_EDGE(K, S, aligned, ragged) \
    (!(aligned) ? K<S, false, true> : (ragged) ? K<S, true, true> : K<S, true, false>)

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
