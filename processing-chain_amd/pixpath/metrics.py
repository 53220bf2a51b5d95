"""Full-reference PSNR / SSIM of a PVS against its source (spec PP-METRIC-1).

The step a user of the chain takes right after p03: how far the AVPVS is from
the SRC, per frame.  The reference has no code for it (its image builds FFmpeg
with libvmaf for the purpose); the numbers are modelled on FFmpeg's vf_psnr
and vf_ssim and their parity with FFmpeg is unpinned.  The sums
run on the MI355X (pp_metrics) over the decoded frames both files' readers
already put into HBM; everything derived from them (MSE, PSNR, the frame and
clip values) is host arithmetic in this module.

The optional measurements that ride on the same resident frames (MS-SSIM, VIF,
ADM, motion, banding, CIEDE2000, PSNR-HVS) are the entries of FEATURES: summarize,
metrics_of_files, report and `cli metrics` loop over that table.
"""
import collections
import os

import numpy as np

from . import adm as _adm, banding as _banding, ciede as _ciede, formats, motion as _motion, msssim as _msssim, \
    psnrhvs as _psnrhvs, vif as _vif
from .clips import clip_pair, crop_window, host_array, json_value, map_entries, nan_mean  # noqa: F401

PLANES = ("y", "u", "v")
# kernel geometry (csrc/metrics.hip), for tests that place sizes on its seams
LANE_BYTES = 16   # kMetLaneBytes: bytes a lane loads per row and input
OWN_LANES = 63    # kMetOwnLanes: lanes of a wave that own blocks
WAVES = 4         # kMetWaves: waves per workgroup
BAND_ROWS = 64    # 4 * kBandBlocks: sample rows of a band


# One optional measurement of `cli metrics`.
#   name       the keyword of metrics_of_files that asks for it, and `--name` of `cli metrics`
#   terms      the keyword of summarize that takes its terms
#   enqueue    (ops, win, d, idx, carried, options) -> (tensors, carried): one batch's GPU calls.  ``ops``:
#              pixpath.ops (it needs torch: only metrics_of_files imports it), ``win``: the resident reference
#              frames, ``d``: the distorted batch, ``idx``: the frame of ``win`` shown with every frame of ``d``,
#              ``carried``: what the call before returned second (None at first), ``options``: metrics_of_files'
#              other keywords by name.  ``tensors``: a tuple of device tensors
#   empty      (trailing shape, dtype) of each of those tensors: what a clip without a frame has
#   summarize  (terms, w, h, matched, fmt, options) -> the per-frame arrays by key plus ``mean``, the clip values by
#              key.  ``terms``: the host array of the whole clip (a tuple of them where enqueue returns several),
#              ``fmt``: the frames' format, ``options``: summarize's option keywords by name
#   flat, rows the per-frame keys report prints as a list and as a list of rows; flat[0] marks a result that has it
Feature = collections.namedtuple("Feature", "name terms enqueue empty summarize flat rows")


def _frame_pairs(op):
    """enqueue of a measurement of every frame pair that carries nothing: ops.<op>."""
    def enqueue(ops, win, d, idx, carried, options):
        return (getattr(ops, op)(win, d, ref_index=idx),), None
    return enqueue


def _enqueue_motion(ops, win, d, idx, held, options):
    sad = ops.motion(win, index=idx, prev=held)
    # the window may be rebuilt before the next batch: a copy, not a view
    return (sad,), win.view(0)[int(idx[-1]):int(idx[-1]) + 1].clone()


def _enqueue_banding(ops, win, d, idx, carried, options):
    return (ops.banding(d), ops.banding(win, index=idx)), None


def _enqueue_ciede(ops, win, d, idx, carried, options):
    return (ops.ciede(win, d, ref_index=idx, weights=options["ciede_weights"] or _ciede.WEIGHTS),), None


def _enqueue_psnr_hvs(ops, win, d, idx, carried, options):
    return (ops.psnr_hvs(win, d, ref_index=idx, step=options["hvs_step"] or _psnrhvs.STEPS[0]),), None


def _summarize_banding(terms, w, h, matched, fmt, options):
    bd, br = (_banding.pool(t)[0] for t in terms)
    res = {"banding_y": bd, "banding_ref_y": br, "banding_added_y": bd - br}
    if matched is not None:
        for v in res.values():
            v[~matched] = np.nan
    res["mean"] = {key: nan_mean(v) for key, v in res.items()}
    return res


# In this order: it is the order of the GPU calls of a batch, of the keys of ``mean`` and of the printed line.
FEATURES = (
    # The luma MS-SSIM and Gaussian-window SSIM of every frame pair (spec PP-MSSSIM-1, ops.ms_ssim: [N, 5, 2]):
    # ``ms_ssim_y``, ``ssim_gauss_y`` [N] and their clip means, ``cs_scales_y`` and ``ssim_scales_y`` [N, 5]
    # (msssim.summarize).
    Feature("ms_ssim", "ms_terms", _frame_pairs("ms_ssim"), (((5, 2), np.float64),),
            lambda t, w, h, matched, fmt, options: _msssim.summarize(t, matched),
            ("ms_ssim_y", "ssim_gauss_y"), ("cs_scales_y", "ssim_scales_y")),
    # The luma VIF and its four per-scale values of every frame pair (spec PP-VIF-1, ops.vif: [N, 4, 2]):
    # ``vif_y`` [N] and ``vif_scales_y`` [N, 4] and their clip means (vif.summarize).
    Feature("vif", "vif_terms", _frame_pairs("vif"), (((4, 2), np.float64),),
            lambda t, w, h, matched, fmt, options: _vif.summarize(t, matched), ("vif_y",), ("vif_scales_y",)),
    # The luma ADM (adm2) and its four per-scale values of every frame pair (spec PP-ADM-1, ops.adm: [N, 4, 6]):
    # ``adm2_y`` [N] and ``adm_scales_y`` [N, 4] and their clip means (adm.summarize).
    Feature("adm", "adm_terms", _frame_pairs("adm"), (((4, 6), np.float64),),
            lambda t, w, h, matched, fmt, options: _adm.summarize(t, w, h, matched), ("adm2_y",), ("adm_scales_y",)),
    # The motion and motion2 of the reference frames as shown (spec PP-MOTION-1, ops.motion on the resident
    # reference window with the same frame map, after the scaler: uint64 [N]; the luma plane of the last frame a
    # batch shows is kept as the next batch's ``prev``): ``motion_y`` and ``motion2_y`` [N] and their clip means
    # (motion.summarize).  An unmatched frame of an explicit map is read against the held reference frame: its
    # difference is 0 for its neighbours' sake and its own values are NaN.
    Feature("motion", "motion_terms", _enqueue_motion, (((), np.uint64),),
            lambda t, w, h, matched, fmt, options: _motion.summarize(t, w, h, matched), ("motion_y", "motion2_y"), ()),
    # The banding index of every distorted frame, of the reference frame shown with it (spec PP-BAND-1,
    # ops.banding on the resident frames with the same frame map, after the scaler: two [N, 5, 1024]; the window
    # is banding.default_window of the distorted picture) and their difference, what the chain added:
    # ``banding_y``, ``banding_ref_y`` and ``banding_added_y`` [N] and their clip means (banding.pool).
    Feature("banding", "banding_terms", _enqueue_banding, (((_banding.SCALES, _banding.BINS), np.uint32),) * 2,
            _summarize_banding, ("banding_y", "banding_ref_y", "banding_added_y"), ()),
    # The CIEDE2000 colour difference of every frame pair, all three planes (spec PP-CIEDE-1, ops.ciede: [N, 2];
    # the option ``ciede_weights``: kL, kC, kH, default the CIE's 1, 1, 1): ``delta_e``, ``delta_e_max`` and
    # ``ciede2000`` [N] and their clip values (ciede.summarize).
    Feature("ciede", "ciede_terms", _enqueue_ciede, (((2,), np.float64),),
            lambda t, w, h, matched, fmt, options: _ciede.summarize(t, w, h, matched), _ciede.KEYS, ()),
    # PSNR-HVS and PSNR-HVS-M of every frame pair, all three planes (spec PP-HVS-1, ops.psnr_hvs: [N, 3, 2]; the
    # option ``hvs_step``: 8, the published definition and default, or 7): ``mse_hvs_*``, ``mse_hvsm_*``,
    # ``psnr_hvs_*`` and ``psnr_hvsm_*`` for y, u, v and all [N] and their clip values, ``hvs_step`` and
    # ``hvs_blocks`` (psnrhvs.summarize).
    Feature("psnr_hvs", "hvs_terms", _enqueue_psnr_hvs, (((3, 2), np.float64),),
            lambda t, w, h, matched, fmt, options: _psnrhvs.summarize(t, w, h, matched, fmt,
                                                                      options["hvs_step"] or _psnrhvs.STEPS[0]),
            _psnrhvs.KEYS, ()),
)


def _psnr(mse, peak):
    """10 log10(peak^2 / MSE); NaN (absent) where MSE is 0 or undefined."""
    mse = np.asarray(mse, dtype=np.float64)
    out = np.full(mse.shape, np.nan)
    ok = mse > 0
    out[ok] = 10.0 * np.log10(peak * peak / mse[ok])
    return out


def summarize(sse, ssim, fmt, w, h, matched=None, ms_terms=None, vif_terms=None, adm_terms=None,
              motion_terms=None, banding_terms=None, ciede_terms=None, hvs_terms=None, hvs_step=None):
    """Host side of PP-METRIC-1: per-frame arrays ``mse_y/u/v/all``,
    ``psnr_y/u/v/all``, ``ssim_y/u/v/all`` (float64 [N]) from pp_metrics' sums
    (sse [N, 3] integers, ssim [N, 3]), plus ``mean``: the clip values (mean
    MSE, PSNR of the mean MSE, mean SSIM over the frames that have one).
    Identical planes (MSE 0) have no PSNR: NaN.  ``all``: MSE over the samples
    of all planes; SSIM weighted by plane size over the planes whose SSIM is
    defined.  ``matched`` (bool [N], an explicit frame map's): the other frames
    have no reference frame; their rows are NaN and the clip values leave them
    out.  Every ``*_terms`` (only when asked for) is the ``terms`` of an entry
    of FEATURES and adds that entry's per-frame arrays and clip values;
    ``hvs_step`` is the block step ``hvs_terms`` were taken at (default 8)."""
    given = {"ms_terms": ms_terms, "vif_terms": vif_terms, "adm_terms": adm_terms, "motion_terms": motion_terms,
             "banding_terms": banding_terms, "ciede_terms": ciede_terms, "hvs_terms": hvs_terms}
    options = {"hvs_step": hvs_step}
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
    for feature in FEATURES:
        if given[feature.terms] is not None:
            r = feature.summarize(given[feature.terms], w, h, matched, f, options)
            mean.update(r.pop("mean"))
            res.update(r)
    return res


def _clip_arrays(outs, empty):
    """The host array of a whole clip for every (trailing shape, dtype) of
    ``empty``, from the tuples of device tensors its batches gave."""
    return tuple(host_array([o[i] for o in outs], tail, dtype) for i, (tail, dtype) in enumerate(empty))


def metrics_of_files(ref_path, dist_path, batch=32, flags="bicubic", crop=None, crop_from="yuv422p", ref_index=None,
                     ms_ssim=False, vif=False, adm=False, motion=False, banding=False, ciede=False,
                     ciede_weights=None, psnr_hvs=False, hvs_step=None):
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

    ``ms_ssim``, ``vif``, ``adm``, ``motion``, ``banding``, ``ciede``,
    ``psnr_hvs``: also the measurement of that ``name`` in FEATURES, on the
    same resident frames with the same frame map; ``ciede_weights`` is ciede's
    option, ``hvs_step`` (8 or 7) psnr_hvs'."""
    import torch

    from . import ops
    from .frames import FrameBatch
    asked = {"ms_ssim": ms_ssim, "vif": vif, "adm": adm, "motion": motion, "banding": banding, "ciede": ciede,
             "psnr_hvs": psnr_hvs}
    if hvs_step is not None:
        _psnrhvs.check_step(hvs_step)
    options = {"ciede_weights": ciede_weights, "hvs_step": hvs_step}
    features = [f for f in FEATURES if asked[f.name]]
    batch = int(batch)
    dev = torch.device("cuda", torch.cuda.current_device())
    with clip_pair(ref_path, dist_path, batch, flags, crop, crop_from) as (ref, dist, dfmt, dw, dh, dists, window):
        outs, k0 = [], 0
        fouts = {f.name: [] for f in features}       # what every batch's enqueue returned, by measurement
        carried = {f.name: None for f in features}   # and what it handed to the next batch's
        explicit = None if ref_index is None else np.asarray(ref_index, dtype=np.int64).reshape(-1)
        last = 0  # explicit map: the reference frame an unmatched distorted frame is read against (and not reported)
        for d in dists:
            if explicit is None:
                m = map_entries(k0, d.n, ref.rate, dist.rate)
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
            window.extend(int(m[-1]) + 1, int(m[0]))  # the reference frames this batch shows, resident
            win, n_ref = window.frames, window.count
            if window.ended and explicit is not None:
                if int(m[-1]) >= n_ref:
                    raise ValueError("ref_index names frame %d of a reference of %d frames" % (int(m[-1]), n_ref))
            elif window.ended:  # the reference's length is known now: the map's true end and clamp
                m = map_entries(k0, d.n, ref.rate, dist.rate, n_in=n_ref)
            if len(m) == 0 or win is None:
                break
            if len(m) < d.n:
                d = FrameBatch(dfmt, dw, dh, len(m), device=d.device, planes=[t[:len(m)] for t in d.planes])
            idx = m - window.first
            outs.append(ops.metrics(win, d, ref_index=idx))
            for f in features:
                tensors, carried[f.name] = f.enqueue(ops, win, d, idx, carried[f.name], options)
                fouts[f.name].append(tensors)
            k0 += d.n
        torch.cuda.current_stream(dev).synchronize()
    sse, ssim = _clip_arrays(outs, (((3,), np.int64), ((3,), np.float64)))
    terms = {}
    for f in features:
        arrays = _clip_arrays(fouts[f.name], f.empty)
        terms[f.terms] = arrays[0] if len(arrays) == 1 else arrays
    matched = None if explicit is None else explicit[:sse.shape[0]] >= 0
    if psnr_hvs:
        terms["hvs_step"] = hvs_step
    return summarize(sse, ssim, dfmt, dw, dh, matched=matched, **terms)


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
    a measurement of FEATURES has its clip values among the former and adds
    its ``flat`` and ``rows`` keys with ``_frames`` to the latter."""
    out = {"ref": os.path.basename(ref_path), "file": os.path.basename(dist_path), "frames": int(res["frames"]),
           "spec": "PP-METRIC-1"}
    for k, v in res["mean"].items():
        out[k] = [json_value(x) for x in v] if isinstance(v, list) else json_value(v)
    if per_frame:
        for kind in ("mse", "psnr", "ssim"):
            for name in PLANES + ("all",):
                key = "%s_%s" % (kind, name)
                out[key + "_frames"] = [json_value(v) for v in res[key]]
        for f in FEATURES:
            if f.flat[0] in res:
                for key in f.flat:
                    out[key + "_frames"] = [json_value(v) for v in res[key]]
                for key in f.rows:
                    out[key + "_frames"] = [[json_value(v) for v in row] for row in res[key]]
    return out
