"""What verifying every pair geometrically costs next to the matching it follows and the consolidation it feeds, measured in ONE process:
    python tools/verify_probe.py [--out profiles/two_view_verify.txt]
A record, not a gate.

Load: that of tools/keypoint_probe.py - all 120 pairs of 16 images of 640 x 640 (fp16, batches of 8, thresholds 0.2 / 0.1, planted
maps), matched once outside the timed windows into match_pairs-style tuples.  Timed forms, after warm-up, 7 windows per form alternating
form by form, reported as median with min .. max:
  (a) matcher.verify_matches end to end: host packing, the one upload, the three launches, the one read back (host clock);
  (b) the three kernels of gf_fundamental_ransac between device events (gf_profile_*, tag fund_ransac), inside form (a)'s calls;
  (c) yardstick: gf_pose_essential_ransac at the same per-pair load and the same number of hypotheses (device events, tag-less: events
      around the call, inputs resident);
  (d) yardstick: matcher.consolidate_matches for the same pairs (host clock);
  (e) yardstick: extract_features + match_features for the same 120 pairs (host clock).
The planted maps are pure image shifts - for a fundamental matrix the degenerate case (every seven matches leave a three-dimensional null
space) - so forms (a) - (c) are also timed on a second load of the same size with an epipolar geometry in it: 120 two-view scenes of
tests/fund_cases.py's generator (vectorised here), as many rows per pair as the matcher returned, 30 % outliers: forms (f), (g), (h).
The refit on the inliers (verify_matches(refit=4): one more launch) is timed beside refit=0 on that second load, in the same process and
the same alternating windows - forms (i), (j) - and, because exact correspondences leave a refit nothing to improve, on a third load: the
second one with 0.5 px of Gaussian noise on both images, forms (k) - (n).  For both the accepted rounds per pair and the mean inlier
count before and after are reported."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = 'cuda:0'
WINDOWS = 7


def line(name, v, unit):
    return f'  {name:<66s} {statistics.median(v):10.3f} {unit}  (min {min(v):.3f} .. max {max(v):.3f})'


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('verify_probe: needs an MI355X')
    import bench
    from feature_cache_probe import planted_images
    from geoformer_amd import _lib, matcher as MT, miopen, ops
    from geoformer_amd.model.full_model import ImageFeatures
    miopen.use_shipped_find_db()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    log(f'verify_probe on {torch.cuda.get_device_name(0)}, torch {torch.__version__}')
    K, batch = 16, 8
    model = bench.build_model('fp16', 0.2, 0.1, DEV)[0]
    i0, i1 = bench.synth_pairs(K // 2, 5, 640, DEV)
    images = torch.cat([i0, i1])
    pc, pf = planted_images(K)
    idx_pairs = [(i, j) for i in range(K) for j in range(i + 1, K)]
    batches = [idx_pairs[s:s + batch] for s in range(0, len(idx_pairs), batch)]
    names = [f'image{k:02d}' for k in range(K)]
    pairs = [(names[i], names[j]) for i, j in idx_pairs]

    def match_pass(collect=None):
        recs = []
        for s in range(0, K, 2 * batch):
            for k, r in enumerate(model.extract_features(images[s:s + 2 * batch]), s):
                recs.append(ImageFeatures(torch.add(pc[k], r.coarse, alpha=0.0), torch.add(pf[k], r.fine, alpha=0.0), r.image_size))
        n = 0
        for bt in batches:
            data = model.match_features([recs[p[0]] for p in bt], [recs[p[1]] for p in bt])
            n += len(data['mkpts0_f'])
            if collect is not None:
                k0, k1 = data['mkpts0_f'].cpu().numpy(), data['mkpts1_f'].cpu().numpy()
                sc, bids = data['mconf'].cpu().numpy(), data['m_bids'].cpu().numpy()
                for q in range(len(bt)):
                    sel = bids == q
                    collect.append((np.concatenate([k0[sel], k1[sel]], axis=1), k0[sel], k1[sel], sc[sel]))
        return n

    results = []
    with torch.no_grad():
        total = match_pass(results)
    iters = ops.FUND_RANSAC_ITERS
    vm = MT.verify_matches(pairs, results, device=DEV)
    log(f'load: {len(pairs)} pairs over {K} images of 640 x 640, fp16, batches of {batch}, thresholds 0.2 / 0.1, planted maps: {total} matches '
        f'({total / len(pairs):.0f} per pair); verification with thr 1 px, min_inliers 15, sc_thres 0.25, {iters} hypotheses per pair')
    log(f'verified {int(vm.verified.sum())} of {len(pairs)} pairs; inliers per pair {int(vm.n_inliers.min())} .. {int(vm.n_inliers.max())} '
        f'(the planted maps are pure image shifts: for F the degenerate case - any seven matches leave a three-dimensional null space, most '
        f'hypotheses fail the pivot test or are ill-conditioned - so few pairs verify here; see the second load)')

    # the second load: one planted two-view geometry per pair, the matcher's row counts, 30 % outliers
    import fund_cases as FC
    rng = np.random.default_rng(2024)
    Ki = np.linalg.inv(FC.K)
    geo = []
    for r in results:
        n = len(r[0])
        R, t, _ = FC.geometry(rng)
        px = np.c_[rng.uniform(0, FC.W, 4 * n + 64), rng.uniform(0, FC.H, 4 * n + 64), np.ones(4 * n + 64)]
        X = (px @ Ki.T) * rng.uniform(3.0, 8.0, (len(px), 1))
        Y = X @ R.T + t
        q = (Y / Y[:, 2:]) @ FC.K.T
        ok = (Y[:, 2] > 0.1) & (q[:, 0] >= 0) & (q[:, 0] < FC.W) & (q[:, 1] >= 0) & (q[:, 1] < FC.H)
        p0, p1 = px[ok][:n, :2], q[ok][:n, :2].copy()
        out = rng.random(len(p0)) < 0.3
        p1[out] = np.c_[rng.uniform(0, FC.W, int(out.sum())), rng.uniform(0, FC.H, int(out.sum()))]
        m = np.c_[p0, p1].astype(np.float32)
        geo.append((m, m[:, :2], m[:, 2:], np.ones(len(m), np.float32)))
    noisy = []
    for g in geo:
        m = (g[0].astype(np.float64) + rng.normal(0, 0.5, g[0].shape)).astype(np.float32)
        noisy.append((m, m[:, :2], m[:, 2:], g[3]))
    vg = MT.verify_matches(pairs, geo, device=DEV)
    log(f'second load: {sum(len(g[0]) for g in geo)} rows in {len(geo)} planted two-view scenes, 30 % outliers: verified {int(vg.verified.sum())} of {len(geo)}, '
        f'inliers per pair {int(vg.n_inliers.min())} .. {int(vg.n_inliers.max())}')

    REFIT = 4
    for name, load in (('second load', geo), ('third load (the second with 0.5 px noise)', noisy)):
        v0, v4 = MT.verify_matches(pairs, load, device=DEV), MT.verify_matches(pairs, load, device=DEV, refit=REFIT)
        log(f'{name}, refit={REFIT}: accepted rounds per pair 0 .. {REFIT}: {np.bincount(v4.rounds, minlength=REFIT + 1).tolist()} pairs; mean inliers '
            f'{v0.n_inliers.mean():.1f} -> {v4.n_inliers.mean():.1f}; verified {int(v0.verified.sum())} -> {int(v4.verified.sum())} of {len(load)}')

    h = _lib.lib()
    kern_ms = []
    kern_geo_ms = []
    kern_refit_ms = {'geo': [], 'noisy0': [], 'noisy4': []}

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    def verify_form(res=None, sink=None, refit=0):
        res, sink = (results, kern_ms) if res is None else (res, sink)
        h.gf_profile_filter(b'fund_ransac')
        h.gf_profile_enable(1)
        ms = timed(lambda: MT.verify_matches(pairs, res, device=DEV, refit=refit))
        tot, cnt, work = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        h.gf_profile_collect(b'fund_ransac', ctypes.byref(tot), ctypes.byref(cnt), ctypes.byref(work))
        h.gf_profile_enable(0)
        h.gf_profile_filter(None)
        sink.append(tot.value / max(cnt.value, 1))
        return ms

    def plain_verify_form(res=None, refit=0):
        return timed(lambda: MT.verify_matches(pairs, results if res is None else res, device=DEV, refit=refit))

    # the essential-matrix RANSAC on the same matches (rows at or above the score threshold), inputs resident, the same number of hypotheses
    def pose_inputs(res, cy):
        ms_all = [np.asarray(r[0], np.float32)[np.asarray(r[3]) >= 0.25] for r in res]
        counts = torch.tensor([sum(len(m) for m in ms_all)] + [len(m) for m in ms_all], dtype=torch.int32, device=DEV)
        mcat = torch.from_numpy(np.concatenate(ms_all)).to(DEV)
        Kmat = torch.tensor([[500.0, 0, 320], [0, 500, cy], [0, 0, 1]], device=DEV).repeat(len(pairs), 1, 1)
        return mcat[:, :2].contiguous(), mcat[:, 2:].contiguous(), counts, Kmat

    pose_in, pose_geo_in = pose_inputs(results, 320.0), pose_inputs(geo, 240.0)

    def pose_form(inp=None):
        mk0, mk1, counts, Kmat = pose_in if inp is None else inp
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        ops.ransac_essential(mk0, mk1, counts, len(pairs), Kmat, Kmat, pixel_thr=1.0, iters=iters)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def consolidate_form():
        return timed(lambda: MT.consolidate_matches(pairs, results, device=DEV))

    def match_form():
        with torch.no_grad():
            return timed(match_pass)

    forms = {'verify': verify_form, 'verify_plain': plain_verify_form, 'pose': pose_form, 'consolidate': consolidate_form, 'match': match_form,
             'geo': lambda: verify_form(geo, kern_geo_ms), 'geo_plain': lambda: plain_verify_form(geo), 'geo_pose': lambda: pose_form(pose_geo_in),
             'geo_refit': lambda: verify_form(geo, kern_refit_ms['geo'], REFIT), 'geo_refit_plain': lambda: plain_verify_form(geo, REFIT),
             'noisy': lambda: verify_form(noisy, kern_refit_ms['noisy0']), 'noisy_plain': lambda: plain_verify_form(noisy),
             'noisy_refit': lambda: verify_form(noisy, kern_refit_ms['noisy4'], REFIT), 'noisy_refit_plain': lambda: plain_verify_form(noisy, REFIT)}
    for fn in forms.values():
        for _ in range(2):
            fn()
    kern_ms.clear()
    kern_geo_ms.clear()
    for v in kern_refit_ms.values():
        v.clear()
    out = {k: [] for k in forms}
    for _ in range(WINDOWS):
        for k, fn in forms.items():
            out[k].append(fn())
    log(f'{WINDOWS} windows per form, the forms alternating; one window = one pass over the {len(pairs)} pairs')
    log(line('(a) verify_matches end to end, kernels under events', out['verify'], 'ms'))
    log(line('(a) verify_matches end to end, no events', out['verify_plain'], 'ms'))
    log(line('(b) rt_prepare, rt_score, rt_final <FundModel> (device events)', kern_ms, 'ms'))
    log(line(f'(c) gf_pose_essential_ransac, same rows, {iters} hypotheses (device events)', out['pose'], 'ms'))
    log(line('(d) consolidate_matches end to end', out['consolidate'], 'ms'))
    log(line('(e) extract_features + match_features, the 120 pairs', out['match'], 'ms'))
    log(line('(f) second load: verify_matches end to end, no events', out['geo_plain'], 'ms'))
    log(line('(g) second load: the three kernels (device events)', kern_geo_ms, 'ms'))
    log(line(f'(h) second load: gf_pose_essential_ransac, {iters} hypotheses (device events)', out['geo_pose'], 'ms'))
    log(line(f'(i) second load: verify_matches(refit={REFIT}) end to end, no events', out['geo_refit_plain'], 'ms'))
    log(line(f'(j) second load: the four kernels, refit={REFIT} (device events)', kern_refit_ms['geo'], 'ms'))
    log(line('(k) third load: verify_matches end to end, no events', out['noisy_plain'], 'ms'))
    log(line('(l) third load: the three kernels (device events)', kern_refit_ms['noisy0'], 'ms'))
    log(line(f'(m) third load: verify_matches(refit={REFIT}) end to end, no events', out['noisy_refit_plain'], 'ms'))
    log(line(f'(n) third load: the four kernels, refit={REFIT} (device events)', kern_refit_ms['noisy4'], 'ms'))
    a, b, c, d, e = (statistics.median(v) for v in (out['verify_plain'], kern_ms, out['pose'], out['consolidate'], out['match']))
    log(f'per pair: verification {1e3 * a / len(pairs):.1f} us end to end, {1e3 * b / len(pairs):.1f} us in its kernels; essential-matrix RANSAC '
        f'{1e3 * c / len(pairs):.1f} us; consolidation {1e3 * d / len(pairs):.1f} us; matching {1e3 * e / len(pairs):.1f} us.  '
        f'verification / matching = {a / e:.4f}; fundamental kernels / essential kernels = {b / c:.3f}')
    f, g, hh = (statistics.median(v) for v in (out['geo_plain'], kern_geo_ms, out['geo_pose']))
    log(f'second load, per pair: verification {1e3 * f / len(pairs):.1f} us end to end, {1e3 * g / len(pairs):.1f} us in its kernels; essential-matrix RANSAC '
        f'{1e3 * hh / len(pairs):.1f} us.  verification / matching = {f / e:.4f}; fundamental kernels / essential kernels = {g / hh:.3f}')
    j, l, n4 = (statistics.median(kern_refit_ms[k]) for k in ('geo', 'noisy0', 'noisy4'))
    log(f'refit={REFIT}, kernels per pair: second load {1e3 * g / len(pairs):.1f} -> {1e3 * j / len(pairs):.1f} us; third load '
        f'{1e3 * l / len(pairs):.1f} -> {1e3 * n4 / len(pairs):.1f} us')


if __name__ == '__main__':
    main()
