"""One synthetic clip's terms of every kind `metrics.summarize` takes, and the
two reports made of them: what tools/gen_metrics_report_golden.py records in
golden/metrics_report.json and test_metrics_report_golden.py rebuilds."""
import numpy as np

FMT, W, H, N = "yuv420p", 33, 33, 5
MATCHED = [True, True, False, True, True]
SEED = 2025


def terms():
    """(sse, ssim, the ``*_terms`` keywords of summarize) of N frames."""
    rng = np.random.default_rng(SEED)
    sse = rng.integers(0, 40000, (N, 3))
    ssim = rng.uniform(0.5, 1.0, (N, 3))
    ssim[1, 2] = np.nan                             # a plane without a window
    ms = rng.uniform(0.6, 1.0, (N, 5, 2))
    ms[1, 4] = np.nan                               # a scale without a window
    vif = rng.uniform(1.0, 900.0, (N, 4, 2))
    adm = rng.uniform(1.0, 5000.0, (N, 4, 6))
    motion = rng.integers(0, 1 << 30, N).astype(np.uint64)
    motion[0] = np.uint64((1 << 64) - 1)            # no frame before the first
    banding = tuple(rng.integers(0, 60, (N, 5, 1024)).astype(np.uint32) for _ in range(2))
    ciede = np.stack([rng.uniform(0.0, 4.0 * W * H, N), rng.uniform(4.0, 30.0, N)], axis=1)
    ciede[3] = 0.0                                  # an identical frame pair
    return sse, ssim, {"ms_terms": ms, "vif_terms": vif, "adm_terms": adm, "motion_terms": motion,
                       "banding_terms": banding, "ciede_terms": ciede}


def reports(metrics):
    """{"plain", "matched"}: report(..., per_frame=True) without and with MATCHED."""
    out = {}
    for name, matched in (("plain", None), ("matched", MATCHED)):
        sse, ssim, kw = terms()
        res = metrics.summarize(sse, ssim, FMT, W, H, matched=matched, **kw)
        out[name] = metrics.report(res, "ref.y4m", "dist.y4m", per_frame=True)
    return out
