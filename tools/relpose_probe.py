"""What the calibrated two-view stage costs next to its two siblings, measured in ONE process:
    python tools/relpose_probe.py [--out profiles/relative_pose.txt]
A record, not a gate.

Load: the epipolar load of tools/verify_probe.py without the matcher in front of it - 120 two-view scenes of tests/fund_cases.py's
generator (vectorised as there, the same generator seed), 1889 rows per pair (the mean the matcher returned there; its per-pair counts
need the model), 30 % outliers, K = fund_cases.K for every image; and the same load with 0.5 px of Gaussian noise on both images, where a
refit has something to improve.  512 hypotheses per pair.  Timed forms, after warm-up, 7 windows per form alternating form by form,
reported as median with min .. max:
  (a) matcher.relative_poses end to end: host packing, the one upload, the launches, the one read back (host clock), refit 0 and 4;
  (b) the launches of gf_relpose_ransac / gf_relpose_ransac_lo between device events (gf_profile_*, tag rel_ransac), inside form (a)'s calls;
  (c) yardstick: gf_pose_essential_ransac on the same rows, the same number of hypotheses (device events around the call, inputs resident);
  (d) yardstick: the three launches of gf_fundamental_ransac on the same rows (tag fund_ransac, inside matcher.verify_matches).
The accepted rounds, the inliers and the pose errors against the planted poses before and after the refit are reported for both loads."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = 'cuda:0'
WINDOWS = 7
PAIRS, ROWS, REFIT = 120, 1889, 4


def line(name, v, unit):
    return f'  {name:<74s} {statistics.median(v):10.3f} {unit}  (min {min(v):.3f} .. max {max(v):.3f})'


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('relpose_probe: needs an MI355X')
    import fund_cases as FC
    import pose_cases as PC
    from geoformer_amd import _lib, matcher as MT, ops
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    log(f'relpose_probe on {torch.cuda.get_device_name(0)}, torch {torch.__version__}')
    rng = np.random.default_rng(2024)
    Ki = np.linalg.inv(FC.K)
    geo, poses = [], []
    for _ in range(PAIRS):
        n = ROWS
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
        poses.append((R, t))
    noisy = []
    for g in geo:
        m = (g[0].astype(np.float64) + rng.normal(0, 0.5, g[0].shape)).astype(np.float32)
        noisy.append((m, m[:, :2], m[:, 2:], g[3]))
    names = [f'image{k:03d}' for k in range(2 * PAIRS)]
    pairs = [(names[2 * k], names[2 * k + 1]) for k in range(PAIRS)]
    intr = {n: FC.K for n in names}
    iters = ops.REL_RANSAC_ITERS
    log(f'load: {sum(len(g[0]) for g in geo)} rows in {PAIRS} planted two-view scenes ({ROWS} per pair), 30 % outliers, one K; thr 1 px, '
        f'min_inliers 15, sc_thres 0.25, {iters} hypotheses per pair; the noisy load: the same rows with 0.5 px noise on both images')
    for name, load in (('exact load', geo), ('noisy load', noisy)):
        r0, r4 = MT.relative_poses(pairs, load, intr, device=DEV), MT.relative_poses(pairs, load, intr, device=DEV, refit=REFIT)
        e0 = np.array([PC.pose_errors(r0.R[k], r0.t[k], *poses[k]) for k in range(PAIRS)])
        e4 = np.array([PC.pose_errors(r4.R[k], r4.t[k], *poses[k]) for k in range(PAIRS)])
        log(f'{name}: verified {int(r0.verified.sum())} -> {int(r4.verified.sum())} of {PAIRS} with refit={REFIT}; accepted rounds per pair 0 .. {REFIT}: '
            f'{np.bincount(r4.rounds, minlength=REFIT + 1).tolist()} pairs; mean inliers {r0.n_inliers.mean():.1f} -> {r4.n_inliers.mean():.1f}; median '
            f'rotation error {np.median(e0[:, 0]):.4f} -> {np.median(e4[:, 0]):.4f} deg, translation direction {np.median(e0[:, 1]):.4f} -> '
            f'{np.median(e4[:, 1]):.4f} deg')

    h = _lib.lib()
    kern = {k: [] for k in ('geo0', 'geo4', 'noisy0', 'noisy4', 'fund')}

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    def under_events(tag, sink, fn):
        h.gf_profile_filter(tag)
        h.gf_profile_enable(1)
        ms = timed(fn)
        tot, cnt, work = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        h.gf_profile_collect(tag, ctypes.byref(tot), ctypes.byref(cnt), ctypes.byref(work))
        h.gf_profile_enable(0)
        h.gf_profile_filter(None)
        sink.append(tot.value / max(cnt.value, 1))
        return ms

    ms_all = [g[0] for g in geo]
    counts = torch.tensor([sum(len(m) for m in ms_all)] + [len(m) for m in ms_all], dtype=torch.int32, device=DEV)
    mcat = torch.from_numpy(np.concatenate(ms_all)).to(DEV)
    mk0, mk1 = mcat[:, :2].contiguous(), mcat[:, 2:].contiguous()
    Kmat = torch.tensor(FC.K, dtype=torch.float32, device=DEV).repeat(PAIRS, 1, 1)

    def pose_form():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        ops.ransac_essential(mk0, mk1, counts, PAIRS, Kmat, Kmat, pixel_thr=1.0, iters=iters)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def rel(load, refit):
        return lambda: MT.relative_poses(pairs, load, intr, device=DEV, refit=refit)

    forms = {'geo0_ev': lambda: under_events(b'rel_ransac', kern['geo0'], rel(geo, 0)), 'geo0': lambda: timed(rel(geo, 0)),
             'geo4_ev': lambda: under_events(b'rel_ransac', kern['geo4'], rel(geo, REFIT)), 'geo4': lambda: timed(rel(geo, REFIT)),
             'noisy0_ev': lambda: under_events(b'rel_ransac', kern['noisy0'], rel(noisy, 0)), 'noisy0': lambda: timed(rel(noisy, 0)),
             'noisy4_ev': lambda: under_events(b'rel_ransac', kern['noisy4'], rel(noisy, REFIT)), 'noisy4': lambda: timed(rel(noisy, REFIT)),
             'pose': pose_form,
             'fund_ev': lambda: under_events(b'fund_ransac', kern['fund'], lambda: MT.verify_matches(pairs, geo, device=DEV, iters=iters))}
    for fn in forms.values():
        for _ in range(2):
            fn()
    for v in kern.values():
        v.clear()
    out = {k: [] for k in forms}
    for _ in range(WINDOWS):
        for k, fn in forms.items():
            out[k].append(fn())
    log(f'{WINDOWS} windows per form, the forms alternating; one window = one pass over the {PAIRS} pairs')
    log(line('(a) exact load: relative_poses end to end, no events', out['geo0'], 'ms'))
    log(line('(b) exact load: rt_prepare, rt_score, rt_final, rt_pose <RelModel> (device events)', kern['geo0'], 'ms'))
    log(line(f'(a) exact load: relative_poses(refit={REFIT}) end to end, no events', out['geo4'], 'ms'))
    log(line(f'(b) exact load: the five launches, refit={REFIT} (device events)', kern['geo4'], 'ms'))
    log(line('(a) noisy load: relative_poses end to end, no events', out['noisy0'], 'ms'))
    log(line('(b) noisy load: the four launches (device events)', kern['noisy0'], 'ms'))
    log(line(f'(a) noisy load: relative_poses(refit={REFIT}) end to end, no events', out['noisy4'], 'ms'))
    log(line(f'(b) noisy load: the five launches, refit={REFIT} (device events)', kern['noisy4'], 'ms'))
    log(line(f'(c) exact load: gf_pose_essential_ransac, {iters} hypotheses (device events)', out['pose'], 'ms'))
    log(line(f'(d) exact load: the three launches of gf_fundamental_ransac, {iters} hypotheses (device events)', kern['fund'], 'ms'))
    a, c, d = (statistics.median(v) for v in (kern['geo0'], out['pose'], kern['fund']))
    lo, hi = min(kern['geo0']) / max(out['pose']), max(kern['geo0']) / min(out['pose'])
    log(f'exact load, launches per pair: calibrated stage {1e3 * a / PAIRS:.1f} us, gf_pose_essential_ransac {1e3 * c / PAIRS:.1f} us, '
        f'gf_fundamental_ransac {1e3 * d / PAIRS:.1f} us.  calibrated / gf_pose_essential_ransac = {a / c:.3f} (over the windows {lo:.3f} .. {hi:.3f}); '
        f'calibrated / fundamental = {a / d:.2f}')
    b0, b4 = statistics.median(kern['noisy0']), statistics.median(kern['noisy4'])
    log(f'refit={REFIT}, launches per pair: exact load {1e3 * a / PAIRS:.1f} -> {1e3 * statistics.median(kern["geo4"]) / PAIRS:.1f} us; noisy load '
        f'{1e3 * b0 / PAIRS:.1f} -> {1e3 * b4 / PAIRS:.1f} us')


if __name__ == '__main__':
    main()
