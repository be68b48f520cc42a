"""What localising queries costs, measured in ONE process:
    python tools/localize_probe.py [--out profiles/localize.txt]
A record, not a gate.

Load: 120 queries, one database pair each, about 1900 rows per query (tests/abspose_cases.py's scene generator behind a synthetic 96 x 128
database 3-D map per pair: the 3-D side of every row comes out of the lookup kernel), 30 % outliers, 0.5 px of Gaussian noise on the query
pixels, 512 hypotheses, thr 2 px.  Timed forms, after warm-up, 7 windows per form alternating form by form, median with min .. max:
  (a) matcher.localize_queries end to end: host packing, the map uploads, the one upload, the lookup, the three launches, the one read
      back (host clock);
  (b) the three kernels of gf_abspose_ransac between device events (gf_profile_*, tag abspose_ransac), inside form (a)'s calls;
  (c), (d) the same with refit=4 (four kernels);
  (e) yardstick: the three kernels of gf_fundamental_ransac on planted two-view scenes of the same row counts, 30 % outliers, 512
      hypotheses (tag fund_ransac)."""
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
HM, WM = 96, 128


def line(name, v, unit):
    return f'  {name:<66s} {statistics.median(v):10.3f} {unit}  (min {min(v):.3f} .. max {max(v):.3f})'


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--queries', type=int, default=120)
    ap.add_argument('--rows', type=int, default=1900)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('localize_probe: needs an MI355X')
    import abspose_cases as AC
    import fund_cases as FC
    from geoformer_amd import _lib, matcher as MT, ops
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    log(f'localize_probe on {torch.cuda.get_device_name(0)}, torch {torch.__version__}')
    rng = np.random.default_rng(2025)
    Q, THR, REFIT, iters = args.queries, 2.0, 4, ops.ABS_RANSAC_ITERS
    pairs, results, maps, intr, two_view = [], [], {}, {}, []
    y, x = np.mgrid[0:HM, 0:WM].astype(np.float64)
    for q in range(Q):
        n = int(rng.integers(args.rows - 100, args.rows + 100))
        R, t = AC.geometry(rng)
        u, v = 20 + 4.7 * x + 0.3 * y, 15 + 4.7 * y - 0.2 * x                      # the database pixel's place in the 640 x 480 query
        depth = 5 + 0.02 * x + 0.01 * y + 0.6 * np.sin(0.15 * x + q) * np.cos(0.1 * y)
        Xc = np.stack([(u - AC.K[0, 2]) / AC.K[0, 0], (v - AC.K[1, 2]) / AC.K[1, 1], np.ones_like(u)], -1) * depth[..., None]
        xyz = ((Xc - t) @ R).astype(np.float32)
        db = np.c_[rng.uniform(0, WM - 1, n), rng.uniform(0, HM - 1, n)].astype(np.float32)
        dmap = torch.from_numpy(xyz).to(DEV)
        X = ops.xyz_lookup(ops.xyz_map_table([dmap], DEV), torch.tensor([0, n], dtype=torch.int32, device=DEV),
                           torch.from_numpy(db).to(DEV)).cpu().numpy().astype(np.float64)
        Y = X @ R.T + t
        px = (Y[:, :2] / Y[:, 2:3]) * [AC.K[0, 0], AC.K[1, 1]] + [AC.K[0, 2], AC.K[1, 2]] + rng.normal(0, 0.5, (n, 2))
        out = rng.random(n) < 0.3
        px[out] = np.c_[rng.uniform(0, AC.W, int(out.sum())), rng.uniform(0, AC.H, int(out.sum()))]
        m = np.c_[px, db].astype(np.float32)
        name, dname = f'query{q:03d}', f'db{q:03d}'
        pairs.append((name, dname)); results.append((m, m[:, :2], m[:, 2:], np.ones(n, np.float32)))
        maps[dname] = xyz; intr[name] = AC.K
        # the yardstick's rows: a planted two-view scene of the same size
        Rf, tf, _ = FC.geometry(rng)
        p0 = np.c_[rng.uniform(0, FC.W, n), rng.uniform(0, FC.H, n), np.ones(n)]
        Yf = ((p0 @ np.linalg.inv(FC.K).T) * rng.uniform(3.0, 8.0, (n, 1))) @ Rf.T + tf
        p1 = ((Yf / Yf[:, 2:]) @ FC.K.T)[:, :2]
        p1[out] = np.c_[rng.uniform(0, FC.W, int(out.sum())), rng.uniform(0, FC.H, int(out.sum()))]
        mf = np.c_[p0[:, :2], p1].astype(np.float32)
        two_view.append((mf, mf[:, :2], mf[:, 2:], np.ones(n, np.float32)))
    M = sum(len(r[0]) for r in results)
    l0 = MT.localize_queries(pairs, results, intr, maps, thr=THR, device=DEV)
    l4 = MT.localize_queries(pairs, results, intr, maps, thr=THR, device=DEV, refit=REFIT)
    log(f'load: {Q} queries, {M} rows ({M / Q:.0f} per query), one {HM} x {WM} 3-D map per query, 30 % outliers, 0.5 px noise; thr {THR} px, '
        f'{iters} hypotheses per query')
    log(f'localised {int(l0.localized.sum())} of {Q}; inliers per query {int(l0.n_inliers.min())} .. {int(l0.n_inliers.max())}; refit={REFIT}: accepted '
        f'rounds per query 0 .. {REFIT}: {np.bincount(l4.rounds, minlength=REFIT + 1).tolist()}, mean inliers {l0.n_inliers.mean():.1f} -> {l4.n_inliers.mean():.1f}')
    h = _lib.lib()
    kern = {'abs0': [], 'abs4': [], 'fund': []}

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

    forms = {'loc0_ev': lambda: under_events(b'abspose_ransac', kern['abs0'], lambda: MT.localize_queries(pairs, results, intr, maps, thr=THR, device=DEV)),
             'loc0': lambda: timed(lambda: MT.localize_queries(pairs, results, intr, maps, thr=THR, device=DEV)),
             'loc4_ev': lambda: under_events(b'abspose_ransac', kern['abs4'],
                                             lambda: MT.localize_queries(pairs, results, intr, maps, thr=THR, device=DEV, refit=REFIT)),
             'loc4': lambda: timed(lambda: MT.localize_queries(pairs, results, intr, maps, thr=THR, device=DEV, refit=REFIT)),
             'fund_ev': lambda: under_events(b'fund_ransac', kern['fund'], lambda: MT.verify_matches(pairs, two_view, device=DEV, iters=iters))}
    for fn in forms.values():
        for _ in range(2):
            fn()
    for v in kern.values():
        v.clear()
    out = {k: [] for k in forms}
    for _ in range(WINDOWS):
        for k, fn in forms.items():
            out[k].append(fn())
    log(f'{WINDOWS} windows per form, the forms alternating; one window = one pass over the {Q} queries')
    log(line('(a) localize_queries end to end, no events', out['loc0'], 'ms'))
    log(line('(b) rt_prepare, rt_score, rt_final <AbsModel> (device events)', kern['abs0'], 'ms'))
    log(line(f'(c) localize_queries(refit={REFIT}) end to end, no events', out['loc4'], 'ms'))
    log(line(f'(d) the four kernels, refit={REFIT} (device events)', kern['abs4'], 'ms'))
    log(line(f'(e) gf_fundamental_ransac, same row counts, {iters} hypotheses: three kernels', kern['fund'], 'ms'))
    a, b, c, d, e = (statistics.median(v) for v in (out['loc0'], kern['abs0'], out['loc4'], kern['abs4'], kern['fund']))
    log(f'per query: localisation {1e3 * a / Q:.1f} us end to end, {1e3 * b / Q:.1f} us in its kernels; refit={REFIT}: {1e3 * c / Q:.1f} / {1e3 * d / Q:.1f} us; '
        f'absolute-pose kernels / fundamental kernels = {b / e:.3f}')


if __name__ == '__main__':
    main()
