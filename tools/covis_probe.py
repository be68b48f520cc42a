"""What the covisibility clustering and the device row path of sparse localisation cost, measured in ONE process:
    python tools/covis_probe.py [--out profiles/covis_localize.txt]
A record, not a gate.

Load: the triangulation probe's database - 16 images on an arc, all 120 pairs, 12,000 planted points of which every image sees a random 39 %,
0.5 px of noise, a pair holds 80 % of the points both images see - plus 8 queries between the database cameras, each paired with 10 database
images drawn at random (80 % of the points both see per pair).  The database is triangulated once from its own pairs (thr 4 px, refit 2).
Localisation: thr 12 px, 512 hypotheses, refit 2.  Timed forms, after warm-up, 7 windows per form alternating form by form, median with
min .. max (host clock around a synchronised call unless stated):
  (a) matcher._sparse_rows: today's rows, on the host;
  (b) the device row path: matcher._covis_tables + matcher._device_rows (bookkeeping, the one upload, cluster kernel off, row kernel, sorts,
      the read of the sizes), the rows left on the device;
  (c) the covis_cluster kernel alone between device events (gf_profile_*, tag covis_cluster), inside form (e)'s call;
  (d) localize_queries_sparse end to end with both flags off, (e) with covis_cluster, (f) with covis_cluster and dedup."""
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


def line(name, v, unit):
    return f'  {name:<66s} {statistics.median(v):10.3f} {unit}  (min {min(v):.3f} .. max {max(v):.3f})'


def planted_scene(n_db, n_q, db_per_q, n_points, see, share, seed):
    """-> (ConsolidatedMatches over database and query images, its database-only part, intrinsics, database poses, query names)"""
    import triangulate_cases as C
    from geoformer_amd import matcher as MT
    rng = np.random.default_rng(seed)
    Kd, Rd, td = C.make_cameras(n_db, seed)
    Kq, Rq, tq = C.make_cameras(n_q, seed + 1)
    K, R, t = np.concatenate([Kd, Kq]), np.concatenate([Rd, Rq]), np.concatenate([td, tq])
    X = np.c_[rng.uniform(-2, 2, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(5, 9, n_points)]
    names = [f'db{i:02d}.png' for i in range(n_db)] + [f'query{i:02d}.png' for i in range(n_q)]
    kp_of_point, keypoints = [], []
    for i in range(n_db + n_q):
        seen = np.flatnonzero(rng.random(n_points) < see)
        Y = X[seen] @ R[i].T + t[i]
        k = np.asarray(K[i], np.float64)
        uv = np.c_[k[0] * Y[:, 0] / Y[:, 2] + k[2], k[4] * Y[:, 1] / Y[:, 2] + k[5]] + rng.normal(0, 0.5, (len(seen), 2))
        idx = np.full(n_points, -1, np.int64)
        idx[seen] = np.arange(len(seen))
        kp_of_point.append(idx), keypoints.append(uv.astype(np.float32))
    idx = [(i, j) for i in range(n_db) for j in range(i + 1, n_db)]
    n_db_pairs = len(idx)
    for q in range(n_q):
        idx += [(n_db + q, int(d)) for d in np.sort(rng.choice(n_db, db_per_q, replace=False))]
    matches = []
    for i, j in idx:
        both = np.flatnonzero((kp_of_point[i] >= 0) & (kp_of_point[j] >= 0))
        both = both[rng.random(len(both)) < share]
        matches.append(np.c_[kp_of_point[i][both], kp_of_point[j][both]].astype(np.int32))
    cm = MT.ConsolidatedMatches(names, keypoints, np.array(idx, np.int32), matches)
    cm_db = cm._replace(pair_images=cm.pair_images[:n_db_pairs], matches=matches[:n_db_pairs])
    return (cm, cm_db, {n: K[i].reshape(3, 3) for i, n in enumerate(names)}, {n: (R[i], t[i]) for i, n in enumerate(names[:n_db])}, names[n_db:],
            {n: (R[i], t[i]) for i, n in enumerate(names)})


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--points', type=int, default=12000)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('covis_probe: needs an MI355X')
    import triangulate_cases as C
    from geoformer_amd import _lib, matcher as MT
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    log(f'covis_probe on {torch.cuda.get_device_name(0)}, torch {torch.__version__}')
    THR, REFIT = 12.0, 2
    cm, cm_db, intr, db_poses, queries, poses = planted_scene(16, 8, 10, args.points, 0.39, 0.8, 2025)
    tt = MT.triangulate(cm_db, intr, db_poses, 4.0, 1.5, 2, 2, device=DEV)
    q_rows = sum(len(m) for m in cm.matches[120:])
    log(f'load: {len(cm.names)} images ({len(queries)} queries), {len(cm.matches)} pairs ({len(cm.matches) - 120} query pairs with {q_rows} match rows), '
        f'{sum(len(k) for k in cm.keypoints)} keypoints, {len(tt.points)} points with {len(tt.obs_image)} observations; thr {THR} px, refit {REFIT}')

    def localize(**kw):
        return MT.localize_queries_sparse(cm, tt, queries, intr, thr=THR, refit=REFIT, device=DEV, **kw)

    def device_rows():
        tb = MT._covis_tables(cm, tt, queries)
        with torch.cuda.device(DEV):
            return MT._device_rows(cm, tt, queries, intr, tb, DEV, False, False)

    p2d, p3d = MT._sparse_rows(cm, tt, queries)[:2]
    fin = np.isfinite(p3d).all(1)
    rows = device_rows()[3]
    same = rows['p2d'].cpu().numpy().tobytes() == p2d[fin].tobytes() and rows['p3d'].cpu().numpy().tobytes() == p3d[fin].tobytes()
    off, on, both = localize(), localize(covis_cluster=True), localize(covis_cluster=True, dedup=True)
    err = lambda lq: max(float(np.linalg.norm(C.centre_of(lq.R[k], lq.t[k]) - C.centre_of(*poses[n]))) for k, n in enumerate(lq.names))  # noqa: E731
    log(f'rows: {len(p2d)} on the host ({int((~fin).sum())} without a point), {rows["M"]} on the device, device == host rows: {same}; clusters per '
        f'query {on.n_clusters.tolist()}; inliers off {off.n_inliers.tolist()}, clustered {on.n_inliers.tolist()}, clustered + dedup '
        f'{both.n_inliers.tolist()}; largest camera-centre error {err(off):.5f} / {err(on):.5f} / {err(both):.5f} units')
    h = _lib.lib()
    kern = []

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    def under_events():
        h.gf_profile_filter(b'covis_cluster')
        h.gf_profile_enable(1)
        ms = timed(lambda: localize(covis_cluster=True))
        tot, cnt, work = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        h.gf_profile_collect(b'covis_cluster', ctypes.byref(tot), ctypes.byref(cnt), ctypes.byref(work))
        h.gf_profile_enable(0)
        h.gf_profile_filter(None)
        kern.append(tot.value / max(cnt.value, 1))
        return ms

    forms = {'host_rows': lambda: timed(lambda: MT._sparse_rows(cm, tt, queries)), 'device_rows': lambda: timed(device_rows), 'cluster_ev': under_events,
             'off': lambda: timed(localize), 'on': lambda: timed(lambda: localize(covis_cluster=True)),
             'both': lambda: timed(lambda: localize(covis_cluster=True, dedup=True))}
    for fn in forms.values():
        for _ in range(2):
            fn()
    kern.clear()
    out = {k: [] for k in forms}
    for _ in range(WINDOWS):
        for k, fn in forms.items():
            out[k].append(fn())
    log(f'{WINDOWS} windows per form, the forms alternating; one window = one pass over the whole load')
    log(line('(a) matcher._sparse_rows: the rows on the host', out['host_rows'], 'ms'))
    log(line('(b) bookkeeping + upload + cluster kernel (off) + row kernel + sorts', out['device_rows'], 'ms'))
    log(line('(c) covis_cluster kernel, 8 workgroups (device events)', kern, 'ms'))
    log(line('(d) localize_queries_sparse end to end, flags off', out['off'], 'ms'))
    log(line('(e) localize_queries_sparse end to end, covis_cluster', out['on'], 'ms'))
    log(line('(f) localize_queries_sparse end to end, covis_cluster + dedup', out['both'], 'ms'))


if __name__ == '__main__':
    main()
