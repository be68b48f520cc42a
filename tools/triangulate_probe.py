"""What triangulating the database tracks costs, measured in ONE process:
    python tools/triangulate_probe.py [--out profiles/triangulate.txt]
A record, not a gate.

Load: the keypoint probe's scale - 16 images, all 120 pairs, about 75 k keypoints - with planted poses: 16 cameras on an arc
(tests/triangulate_cases.py), 12,000 planted points of which every image sees a random 39 %, 0.5 px of Gaussian noise per observation, a
pair holds 80 % of the points both images see, and 1 % of a pair's rows are mismatches (they join two tracks: conflicts).  thr 4 px, 1.5
degrees, at least 2 observations, refit 2.  Timed forms, after warm-up, 7 windows per form alternating form by form, median with min .. max:
  (a) matcher.triangulate end to end: host packing, the one upload, tracks, triangulation, the one read back, host assembly (host clock);
  (b) gf_track_link's two kernels and (c) gf_track_flatten's kernel between device events (gf_profile_*, tags track_link, track_flatten);
  (d) the two launches tri_hypotheses + tri_finish between device events (tag triangulate), each inside form (a)'s calls;
  (e) the serial host build (csrc/host/tri_host.cpp) on the same input: labelling + track list, and the triangulation (host clock)."""
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


def planted_matches(n_images, n_points, see, share, wrong, seed):
    """-> (ConsolidatedMatches, intrinsics, poses): keypoints are the noisy projections of the points an image sees"""
    import triangulate_cases as C
    from geoformer_amd import matcher as MT
    rng = np.random.default_rng(seed)
    K, R, t = C.make_cameras(n_images, seed)
    X = np.c_[rng.uniform(-2, 2, n_points), rng.uniform(-1.5, 1.5, n_points), rng.uniform(5, 9, n_points)]
    names = [f'db{i:02d}.png' for i in range(n_images)]
    kp_of_point, keypoints = [], []
    for i in range(n_images):
        seen = np.flatnonzero(rng.random(n_points) < see)
        Y = X[seen] @ R[i].T + t[i]
        k = np.asarray(K[i], np.float64)
        uv = np.c_[k[0] * Y[:, 0] / Y[:, 2] + k[2], k[4] * Y[:, 1] / Y[:, 2] + k[5]] + rng.normal(0, 0.5, (len(seen), 2))
        idx = np.full(n_points, -1, np.int64)
        idx[seen] = np.arange(len(seen))
        kp_of_point.append(idx), keypoints.append(uv.astype(np.float32))
    pairs, matches = [], []
    for i in range(n_images):
        for j in range(i + 1, n_images):
            both = np.flatnonzero((kp_of_point[i] >= 0) & (kp_of_point[j] >= 0))
            both = both[rng.random(len(both)) < share]
            m = np.c_[kp_of_point[i][both], kp_of_point[j][both]].astype(np.int32)
            bad = np.flatnonzero(rng.random(len(m)) < wrong)
            m[bad, 1] = rng.integers(0, len(keypoints[j]), len(bad))
            pairs.append((i, j)), matches.append(m)
    cm = MT.ConsolidatedMatches(names, keypoints, np.array(pairs, np.int32), matches)
    return cm, {n: K[i].reshape(3, 3) for i, n in enumerate(names)}, {n: (R[i], t[i]) for i, n in enumerate(names)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--images', type=int, default=16)
    ap.add_argument('--points', type=int, default=12000)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('triangulate_probe: needs an MI355X')
    import triangulate_cases as C
    from geoformer_amd import _lib, matcher as MT
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    log(f'triangulate_probe on {torch.cuda.get_device_name(0)}, torch {torch.__version__}')
    THR, ANGLE, MIN_OBS, REFIT = 4.0, 1.5, 2, 2
    cm, intr, poses = planted_matches(args.images, args.points, 0.39, 0.8, 0.01, 2025)
    n_kp, n_rows = sum(len(k) for k in cm.keypoints), sum(len(m) for m in cm.matches)
    tt = MT.triangulate(cm, intr, poses, THR, ANGLE, MIN_OBS, REFIT, device=DEV)
    log(f'load: {len(cm.names)} images, {len(cm.matches)} pairs, {n_kp} keypoints, {n_rows} match rows, 0.5 px noise, 1 % mismatched rows; thr {THR} px, '
        f'{ANGLE} deg, min_obs {MIN_OBS}, refit {REFIT}')
    # the serial host build on the same input, and the track statistics from it
    n, kp_off, K, R, t, origin, ids, id_off, kps, pim = MT._triangulation_inputs(cm, intr, poses)
    g = {'ids': ids, 'id_off': id_off, 'pair_images': pim, 'kp_off': kp_off, 'n_nodes': int(kp_off[-1])}
    host_tracks_ms, host_tri_ms = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        st, _, toff, oimg, okp, onode = C.host_tracks(g)
        t1 = time.perf_counter()
        rc, ho = C.host_triangulate(toff, oimg, kps[onode], K, R, t, pixel_thr=THR, min_angle_deg=ANGLE, min_obs=MIN_OBS, refit=REFIT)
        t2 = time.perf_counter()
        host_tracks_ms.append(1e3 * (t1 - t0)), host_tri_ms.append(1e3 * (t2 - t1))
    ht = MT._assemble_tracks(n, kp_off, len(toff) - 1, ho['X'], ho['err2'], ho['valid'], ho['conflict'], toff, oimg, okp, ho['inliers'], origin)
    same = ht.points.tobytes() == tt.points.tobytes() and ht.obs_keypoint.tobytes() == tt.obs_keypoint.tobytes()
    lens = np.diff(toff)
    hist = np.bincount(np.minimum(lens, 17), minlength=18)
    slots = int(sum(min(L * (L - 1) // 2, 64) for L, c in zip(lens, ho['conflict']) if not c))
    log(f'tracks: {tt.n_tracks} ({tt.n_conflict} conflicts = {100.0 * tt.n_conflict / max(tt.n_tracks, 1):.2f} %, {tt.n_rejected} rejected), '
        f'{len(tt.points)} points, {len(tt.obs_image)} inlier observations of {len(oimg)}; {slots} hypothesis slots; '
        f'median reprojection error {float(np.median(tt.errors)):.3f} px; device == host build: {same}')
    log('track lengths 2 .. 16, 17+: ' + ' '.join(str(int(v)) for v in hist[2:]))
    h = _lib.lib()
    kern = {'link': [], 'flatten': [], 'tri': []}

    def run():
        return MT.triangulate(cm, intr, poses, THR, ANGLE, MIN_OBS, REFIT, device=DEV)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    def under_events(tag, sink):
        h.gf_profile_filter(tag)
        h.gf_profile_enable(1)
        ms = timed(run)
        tot, cnt, work = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        h.gf_profile_collect(tag, ctypes.byref(tot), ctypes.byref(cnt), ctypes.byref(work))
        h.gf_profile_enable(0)
        h.gf_profile_filter(None)
        sink.append(tot.value / max(cnt.value, 1))
        return ms

    forms = {'e2e': lambda: timed(run), 'link_ev': lambda: under_events(b'track_link', kern['link']),
             'flatten_ev': lambda: under_events(b'track_flatten', kern['flatten']), 'tri_ev': lambda: under_events(b'triangulate', kern['tri'])}
    for fn in forms.values():
        for _ in range(2):
            fn()
    for v in kern.values():
        v.clear()
    out = {k: [] for k in forms}
    for _ in range(WINDOWS):
        for k, fn in forms.items():
            out[k].append(fn())
    log(f'{WINDOWS} windows per form, the forms alternating; one window = one pass over the whole load')
    log(line('(a) matcher.triangulate end to end, no events', out['e2e'], 'ms'))
    log(line('(b) track_init + track_link (device events)', kern['link'], 'ms'))
    log(line('(c) track_flatten (device events)', kern['flatten'], 'ms'))
    log(line('(d) tri_hypotheses + tri_finish (device events)', kern['tri'], 'ms'))
    log(line('(e) serial host build: labelling + track list (3 runs)', host_tracks_ms, 'ms'))
    log(line('(e) serial host build: triangulation (3 runs)', host_tri_ms, 'ms'))


if __name__ == '__main__':
    main()
