"""Full-reference PSNR / SSIM of a PVS against its source (spec PP-METRIC-1).

The step a user of the chain takes right after p03: how far the AVPVS is from
the SRC, per frame.  The reference has no code for it (its image builds FFmpeg
with libvmaf for the purpose); the numbers are modelled on FFmpeg's vf_psnr
and vf_ssim and their parity with FFmpeg is unpinned.  The sums
run on the MI355X (pp_metrics) over the decoded frames both files' readers
already put into HBM; everything derived from them (MSE, PSNR, the frame and
clip values) is host arithmetic in this module.
"""
import os

import numpy as np

from . import formats
from .clips import clip_batches, crop_window, json_value, nan_mean, planar_format  # noqa: F401

PLANES = ("y", "u", "v")
# kernel geometry (csrc/metrics.hip), for tests that place sizes on its seams
LANE_BYTES = 16   # kMetLaneBytes: bytes a lane loads per row and input
OWN_LANES = 63    # kMetOwnLanes: lanes of a wave that own blocks
WAVES = 4         # kMetWaves: waves per workgroup
BAND_ROWS = 64    # 4 * kBandBlocks: sample rows of a band


def _psnr(mse, peak):
    """10 log10(peak^2 / MSE); NaN (absent) where MSE is 0 or undefined."""
    mse = np.asarray(mse, dtype=np.float64)
    out = np.full(mse.shape, np.nan)
    ok = mse > 0
    out[ok] = 10.0 * np.log10(peak * peak / mse[ok])
    return out


def summarize(sse, ssim, fmt, w, h, matched=None, ms_terms=None, vif_terms=None, adm_terms=None,
              motion_terms=None, banding_terms=None, ciede_terms=None):
    """Host side of PP-METRIC-1: per-frame arrays ``mse_y/u/v/all``,
    ``psnr_y/u/v/all``, ``ssim_y/u/v/all`` (float64 [N]) from pp_metrics' sums
    (sse [N, 3] integers, ssim [N, 3]), plus ``mean``: the clip values (mean
    MSE, PSNR of the mean MSE, mean SSIM over the frames that have one).
    Identical planes (MSE 0) have no PSNR: NaN.  ``all``: MSE over the samples
    of all planes; SSIM weighted by plane size over the planes whose SSIM is
    defined.  ``matched`` (bool [N], an explicit frame map's): the other frames
    have no reference frame; their rows are NaN and the clip values leave them
    out.  ``ms_terms`` (pp_ms_ssim's [N, 5, 2], spec PP-MSSSIM-1; only when
    asked for): adds ``ms_ssim_y``, ``ssim_gauss_y`` [N], ``cs_scales_y`` and
    ``ssim_scales_y`` [N, 5] and the clip means of the first two
    (msssim.summarize).  ``vif_terms`` (pp_vif's [N, 4, 2], spec PP-VIF-1; only
    when asked for): adds ``vif_y`` [N] and ``vif_scales_y`` [N, 4] and their
    clip means (vif.summarize).  ``adm_terms`` (pp_adm's [N, 4, 6], spec
    PP-ADM-1; only when asked for): adds ``adm2_y`` [N] and ``adm_scales_y``
    [N, 4] and their clip means (adm.summarize).  ``motion_terms`` (pp_motion's
    [N] of the reference frames as shown, spec PP-MOTION-1; only when asked
    for): adds ``motion_y`` and ``motion2_y`` [N] and their clip means
    (motion.summarize).  ``banding_terms`` (pp_banding's [N, 5, 1024] of the
    distorted frames and of the reference frames as shown, spec PP-BAND-1; only
    when asked for): adds ``banding_y``, ``banding_ref_y`` and their difference
    ``banding_added_y`` [N] and their clip means (banding.pool).
    ``ciede_terms`` (pp_ciede's [N, 2], spec PP-CIEDE-1; only when asked for):
    adds ``delta_e``, ``delta_e_max`` and ``ciede2000`` [N] and their clip
    values (ciede.summarize)."""
    f = formats.fmt(fmt)
    sse = np.asarray(sse).reshape(-1, 3)
    ssim = np.asarray(ssim, dtype=np.float64).reshape(-1, 3)
    size = np.array([r * c for r, c in formats.plane_shapes(f, w, h)], dtype=np.float64)
    peak = float((1 << f.depth) - 1)
    # exact integers up to 2^53: a 2160p 4:4:4 frame of full-range error stays below
    sse = sse.astype(np.float64)
    res = {}
    for p, name in enumerate(PLANES):
        res["mse_" + name] = sse[:, p] / size[p]
        res["ssim_" + name] = ssim[:, p].copy()
    res["mse_all"] = sse.sum(axis=1) / size.sum()
    ok = ~np.isnan(ssim)
    wsum = (ok * size).sum(axis=1)
    num = (np.where(ok, ssim, 0.0) * size).sum(axis=1)
    res["ssim_all"] = np.where(wsum > 0, num / np.where(wsum > 0, wsum, 1.0), np.nan)
    for name in PLANES + ("all",):
        res["psnr_" + name] = _psnr(res["mse_" + name], peak)
    if matched is not None:
        matched = np.asarray(matched, dtype=bool)
        for key in res:
            res[key][~matched] = np.nan
    mean = {}
    for name in PLANES + ("all",):
        m = res["mse_" + name]
        if matched is not None:
            m = m[matched]
        mean["mse_" + name] = float(m.mean()) if m.size else float("nan")
        mean["psnr_" + name] = float(_psnr(mean["mse_" + name], peak))
        mean["ssim_" + name] = nan_mean(res["ssim_" + name])
    res["mean"] = mean
    res["frames"] = int(sse.shape[0])
    if ms_terms is not None:
        from . import msssim
        ms = msssim.summarize(ms_terms, matched)
        mean.update(ms.pop("mean"))
        res.update(ms)
    if vif_terms is not None:
        from . import vif
        vs = vif.summarize(vif_terms, matched)
        mean.update(vs.pop("mean"))
        res.update(vs)
    if adm_terms is not None:
        from . import adm
        ad = adm.summarize(adm_terms, w, h, matched)
        mean.update(ad.pop("mean"))
        res.update(ad)
    if motion_terms is not None:
        from . import motion
        mo = motion.summarize(motion_terms, w, h, matched)
        mean.update(mo.pop("mean"))
        res.update(mo)
    if banding_terms is not None:
        from . import banding
        bd, br = (banding.pool(t)[0] for t in banding_terms)
        for key, v in (("banding_y", bd), ("banding_ref_y", br), ("banding_added_y", bd - br)):
            if matched is not None:
                v[~matched] = np.nan
            res[key] = v
            mean[key] = nan_mean(v)
    if ciede_terms is not None:
        from . import ciede
        ce = ciede.summarize(ciede_terms, w, h, matched)
        mean.update(ce.pop("mean"))
        res.update(ce)
    return res


def _map_entries(k0, n, in_rate, out_rate, n_in=None):
    """vf_fps entries [k0, k0 + n) of the dist <- ref frame map.  Before the
    reference's length is known the map of a long enough clip is used: the two
    agree on every entry below the true clip's end, up to the clamp to its
    last frame."""
    from . import ops
    if n_in is None:
        n_in = int((k0 + n) * in_rate / out_rate) + 4
    return ops.fps_map(n_in, in_rate, out_rate)[k0:k0 + n]


def metrics_of_files(ref_path, dist_path, batch=32, flags="bicubic", crop=None, crop_from="yuv422p", ref_index=None,
                     ms_ssim=False, vif=False, adm=False, motion=False, banding=False, ciede=False,
                     ciede_weights=None):
    """PP-METRIC-1 of the file ``dist_path`` (the PVS) against ``ref_path``
    (the SRC); returns ``summarize``'s dict.  Both are read with the chain's
    own readers (FFV1 AVIs through ffv1.open_avpvs_reader, anything else
    through io.open_reader).  A reference of another size or pixel format is
    first brought to the distorted clip's with ops.Scaler (``flags``); at
    another rate, distorted frame k is compared with the reference frame
    vf_fps would show there (ops.fps_map).  Frames stream through the GPU
    ``batch`` at a time; the comparison ends with the shorter of the distorted
    clip and the rate-converted reference.

    A v210 or UYVY AVI (a CPVS, or an uncompressed SRC) is read by
    io.PackedAviReader and unpacked on the GPU (ops.unpack) to yuv422p10le /
    yuv422p.  ``crop`` = (w, h): the distorted clip is a CPVS canvas and only
    the w x h AVPVS picture inside it is compared, at the offsets the CPVS pad
    put it (crop_window; ``crop_from``: the AVPVS's pixel format, which decides
    the rounding of the offsets -- pass "yuv420p" / "yuv420p10le" for a 4:2:0
    AVPVS).  Without ``crop`` the whole canvas is compared.

    ``ref_index`` (one int per distorted frame, pixpath.align's ``map``)
    replaces the vf_fps map: distorted frame k is compared with reference
    frame ref_index[k], the matched entries never going back; a frame with
    ref_index[k] < 0 has no reference frame: its rows are NaN and the clip
    values leave it out.  The comparison ends with the shorter of the
    distorted clip and the map.

    ``ms_ssim``: also the luma MS-SSIM and Gaussian-window SSIM of every frame
    pair (spec PP-MSSSIM-1, ops.ms_ssim on the same resident frames).

    ``vif``: also the luma VIF and its four per-scale values of every frame
    pair (spec PP-VIF-1, ops.vif on the same resident frames).

    ``adm``: also the luma ADM (adm2) and its four per-scale values of every
    frame pair (spec PP-ADM-1, ops.adm on the same resident frames).

    ``motion``: also the motion and motion2 of the reference frames as shown
    (spec PP-MOTION-1, ops.motion on the resident reference window with the
    same frame map, after the scaler; the luma plane of the last frame shown
    by a batch is kept as the next batch's ``prev``).  An unmatched frame of
    an explicit map is read against the held reference frame: its difference
    is 0 for its neighbours' sake and its own values are NaN.

    ``banding``: also the banding index of every distorted frame, of the
    reference frame shown with it (spec PP-BAND-1, ops.banding on the resident
    frames with the same frame map, after the scaler; the window is
    banding.default_window of the distorted picture) and their difference,
    what the chain added.

    ``ciede``: also the CIEDE2000 colour difference of every frame pair, all
    three planes (spec PP-CIEDE-1, ops.ciede on the same resident frames);
    ``ciede_weights``: kL, kC, kH (default: the CIE's 1, 1, 1)."""
    import torch

    from . import ops
    from .frames import FrameBatch
    batch = int(batch)
    dev = torch.device("cuda", torch.cuda.current_device())
    with clip_batches(ref_path, batch) as (ref, _, refs), \
            clip_batches(dist_path, batch, crop, crop_from, "distorted clip") as (dist, window, dists):
        rfmt, dfmt = planar_format(ref), planar_format(dist)
        dw, dh = (dist.w, dist.h) if window is None else window[2:]
        same = (rfmt.id, ref.w, ref.h) == (dfmt.id, dw, dh)
        scaler = None if same else ops.Scaler(rfmt, ref.w, ref.h, dfmt, dw, dh, flags=flags, device=dev)
        in_rate, out_rate = ref.rate, dist.rate
        win, win0, n_ref, ref_end = None, 0, 0, False  # resident reference frames [win0, n_ref), dist geometry
        outs, terms, vterms, aterms, k0 = [], [], [], [], 0
        bterms, brterms = [], []  # PP-BAND-1: histograms of the distorted frames and of the reference frames as shown
        cterms = []  # PP-CIEDE-1: sum and maximum of every frame pair
        mterms, held = [], None  # PP-MOTION-1: the sums, and a copy of the luma plane of the last frame shown
        explicit = None if ref_index is None else np.asarray(ref_index, dtype=np.int64).reshape(-1)
        last = 0  # explicit map: the reference frame an unmatched distorted frame is read against (and not reported)
        for d in dists:
            if explicit is None:
                m = _map_entries(k0, d.n, in_rate, out_rate)
            else:
                m = explicit[k0:k0 + d.n].copy()
                if len(m) == 0:
                    break
                for i in range(len(m)):
                    if m[i] < 0:
                        m[i] = last
                    elif m[i] < last:
                        raise ValueError("ref_index goes back from %d to %d at frame %d" % (last, m[i], k0 + i))
                    last = int(m[i])
            while not ref_end and n_ref <= int(m[-1]):
                r = next(refs, None)
                if r is None:
                    ref_end = True
                    break
                if scaler is not None:
                    r = scaler(r)
                keep = max(int(m[0]) - win0, 0) if win is not None else 0
                if win is None or keep >= win.n:
                    win, win0 = r, n_ref
                else:
                    k1 = win.n - keep
                    nw = FrameBatch(dfmt, dw, dh, k1 + r.n, device=dev)
                    for p in range(3):
                        nw.view(p)[:k1].copy_(win.view(p)[keep:])
                        nw.view(p)[k1:].copy_(r.view(p))
                    win, win0 = nw, win0 + keep
                n_ref += r.n
            if ref_end and explicit is not None:
                if int(m[-1]) >= n_ref:
                    raise ValueError("ref_index names frame %d of a reference of %d frames" % (int(m[-1]), n_ref))
            elif ref_end:  # the reference's length is known now: the map's true end and clamp
                m = _map_entries(k0, d.n, in_rate, out_rate, n_in=n_ref)
            if len(m) == 0 or win is None:
                break
            if len(m) < d.n:
                d = FrameBatch(dfmt, dw, dh, len(m), device=d.device, planes=[t[:len(m)] for t in d.planes])
            outs.append(ops.metrics(win, d, ref_index=m - win0))
            if ms_ssim:
                terms.append(ops.ms_ssim(win, d, ref_index=m - win0))
            if vif:
                vterms.append(ops.vif(win, d, ref_index=m - win0))
            if adm:
                aterms.append(ops.adm(win, d, ref_index=m - win0))
            if motion:
                mterms.append(ops.motion(win, index=m - win0, prev=held).view(torch.int64))
                # the window may be rebuilt before the next batch: a copy, not a view
                held = win.view(0)[int(m[-1]) - win0:int(m[-1]) - win0 + 1].clone()
            if banding:
                bterms.append(ops.banding(d))
                brterms.append(ops.banding(win, index=m - win0))
            if ciede:
                cterms.append(ops.ciede(win, d, ref_index=m - win0, weights=ciede_weights or (1.0, 1.0, 1.0)))
            k0 += d.n
        torch.cuda.current_stream(dev).synchronize()
    if outs:
        sse = torch.cat([o[0] for o in outs]).cpu().numpy()
        ssim = torch.cat([o[1] for o in outs]).cpu().numpy()
    else:
        sse, ssim = np.zeros((0, 3), np.int64), np.zeros((0, 3))
    ms = None
    if ms_ssim:
        ms = torch.cat(terms).cpu().numpy() if terms else np.zeros((0, 5, 2))
    vt = None
    if vif:
        vt = torch.cat(vterms).cpu().numpy() if vterms else np.zeros((0, 4, 2))
    at = None
    if adm:
        at = torch.cat(aterms).cpu().numpy() if aterms else np.zeros((0, 4, 6))
    mt = None
    if motion:
        mt = torch.cat(mterms).cpu().numpy().view(np.uint64) if mterms else np.zeros((0,), np.uint64)
    bt = None
    if banding:
        from .banding import BINS, SCALES
        bt = tuple(torch.cat(t).cpu().numpy() if t else np.zeros((0, SCALES, BINS), np.uint32) for t in (bterms, brterms))
    ct = None
    if ciede:
        ct = torch.cat(cterms).cpu().numpy() if cterms else np.zeros((0, 2))
    if explicit is None:
        return summarize(sse, ssim, dfmt, dw, dh, ms_terms=ms, vif_terms=vt, adm_terms=at, motion_terms=mt,
                         banding_terms=bt, ciede_terms=ct)
    return summarize(sse, ssim, dfmt, dw, dh, matched=explicit[:sse.shape[0]] >= 0, ms_terms=ms, vif_terms=vt,
                     adm_terms=at, motion_terms=mt, banding_terms=bt, ciede_terms=ct)


VMAF_FEATURE_NAMES = ("adm2", "motion2", "vif_scale0", "vif_scale1", "vif_scale2", "vif_scale3")


def vmaf_features(res, per_frame=False):
    """The six elementary features the published VMAF models take, in
    VMAF_FEATURE_NAMES' order, from a result with VIF, ADM and motion:
    ``vmaf_features`` (the clip means), ``vmaf_feature_names`` and, with
    per_frame, ``vmaf_features_frames`` [N][6]; NaN becomes null.  No model is
    applied: the library ships none."""
    mean = res["mean"]
    out = {"vmaf_features": [json_value(v) for v in [mean["adm2_y"], mean["motion2_y"]] + list(mean["vif_scales_y"])],
           "vmaf_feature_names": list(VMAF_FEATURE_NAMES)}
    if per_frame:
        out["vmaf_features_frames"] = [
            [json_value(v) for v in [a, m] + list(row)]
            for a, m, row in zip(res["adm2_y"], res["motion2_y"], res["vif_scales_y"])]
    return out


def report(res, ref_path, dist_path, per_frame=False):
    """The JSON object `cli metrics` prints: clip values, and with per_frame
    the per-frame lists; NaN and infinite values become null.  A result with
    MS-SSIM (summarize's ms_terms) adds ``ms_ssim_y``, ``ssim_gauss_y`` and,
    per frame, those two and the per-scale means ``cs_scales_y_frames`` /
    ``ssim_scales_y_frames`` ([N][5]).  A result with VIF (summarize's
    vif_terms) adds ``vif_y`` and ``vif_scales_y`` (four values) and, per
    frame, ``vif_y_frames`` and ``vif_scales_y_frames`` ([N][4]).  A result
    with ADM (summarize's adm_terms) adds ``adm2_y`` and ``adm_scales_y`` (four
    values) and, per frame, ``adm2_y_frames`` and ``adm_scales_y_frames``
    ([N][4]).  A result with motion (summarize's motion_terms) adds
    ``motion_y`` and ``motion2_y`` and, per frame, ``motion_y_frames`` and
    ``motion2_y_frames``.  A result with banding (summarize's banding_terms)
    adds ``banding_y``, ``banding_ref_y`` and ``banding_added_y`` and, per
    frame, the three lists with ``_frames``.  A result with CIEDE2000
    (summarize's ciede_terms) adds ``delta_e``, ``delta_e_max`` and
    ``ciede2000`` and, per frame, the three lists with ``_frames``."""
    out = {"ref": os.path.basename(ref_path), "file": os.path.basename(dist_path), "frames": int(res["frames"]),
           "spec": "PP-METRIC-1"}
    for k, v in res["mean"].items():
        out[k] = [json_value(x) for x in v] if isinstance(v, list) else json_value(v)
    if per_frame:
        for kind in ("mse", "psnr", "ssim"):
            for name in PLANES + ("all",):
                key = "%s_%s" % (kind, name)
                out[key + "_frames"] = [json_value(v) for v in res[key]]
        if "ms_ssim_y" in res:
            for key in ("ms_ssim_y", "ssim_gauss_y"):
                out[key + "_frames"] = [json_value(v) for v in res[key]]
            for key in ("cs_scales_y", "ssim_scales_y"):
                out[key + "_frames"] = [[json_value(v) for v in row] for row in res[key]]
        if "vif_y" in res:
            out["vif_y_frames"] = [json_value(v) for v in res["vif_y"]]
            out["vif_scales_y_frames"] = [[json_value(v) for v in row] for row in res["vif_scales_y"]]
        if "adm2_y" in res:
            out["adm2_y_frames"] = [json_value(v) for v in res["adm2_y"]]
            out["adm_scales_y_frames"] = [[json_value(v) for v in row] for row in res["adm_scales_y"]]
        if "motion_y" in res:
            out["motion_y_frames"] = [json_value(v) for v in res["motion_y"]]
            out["motion2_y_frames"] = [json_value(v) for v in res["motion2_y"]]
        if "banding_y" in res:
            for key in ("banding_y", "banding_ref_y", "banding_added_y"):
                out[key + "_frames"] = [json_value(v) for v in res[key]]
        if "delta_e" in res:
            from . import ciede
            out.update(ciede.frames_report(res))
    return out
