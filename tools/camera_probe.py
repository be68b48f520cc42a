"""What removing lens distortion from the matches costs next to the consolidation that follows it, measured in ONE process:
    python tools/camera_probe.py [--out profiles/camera_undistort.txt]

Load: that of tools/keypoint_probe.py - all 120 pairs of 16 images of 640 x 640 (fp16, batches of 8, thresholds 0.2 / 0.1, planted maps),
matched once outside the timed windows into match_pairs-style tuples; every image a SIMPLE_RADIAL camera (f 600, centre 320, k -0.1).
Timed forms, after warm-up, 7 windows per form alternating form by form, reported as median with min .. max:
  (a) matcher.undistort_results end to end: host packing, the one upload, the two launches, the one read back, the tuples (host clock);
  (b) the two launches alone on rows that are on the device, between device events;
  (c) the serial host C++ build (csrc/host/camera_host.cpp) on the same rows, both sides (host clock);
  (d) the yardstick: matcher.consolidate_matches on the same tuples (host clock).
Also reported: rows, rows without a pre-image, and that (a) and (c) agree bit for bit.  A record, not a gate."""
import argparse
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
        raise SystemExit('camera_probe: needs an MI355X')
    import bench
    import camera_cases as CC
    from feature_cache_probe import planted_images
    from geoformer_amd import matcher as MT, miopen, ops
    from geoformer_amd.model.full_model import ImageFeatures
    miopen.use_shipped_find_db()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    log(f'camera_probe on {torch.cuda.get_device_name(0)}, torch {torch.__version__}')
    K, batch = 16, 8
    model = bench.build_model('fp16', 0.2, 0.1, DEV)[0]
    i0, i1 = bench.synth_pairs(K // 2, 5, 640, DEV)
    images = torch.cat([i0, i1])
    pc, pf = planted_images(K)
    idx_pairs = [(i, j) for i in range(K) for j in range(i + 1, K)]
    names = [f'image{k:02d}' for k in range(K)]
    pairs = [(names[i], names[j]) for i, j in idx_pairs]
    cams = {n: MT.Camera('SIMPLE_RADIAL', 640, 640, (600.0, 320.0, 320.0, -0.1)) for n in names}
    results = []
    with torch.no_grad():
        recs = []
        for s in range(0, K, 2 * batch):
            for k, r in enumerate(model.extract_features(images[s:s + 2 * batch]), s):
                recs.append(ImageFeatures(torch.add(pc[k], r.coarse, alpha=0.0), torch.add(pf[k], r.fine, alpha=0.0), r.image_size))
        for s in range(0, len(idx_pairs), batch):
            bt = idx_pairs[s:s + batch]
            data = model.match_features([recs[p[0]] for p in bt], [recs[p[1]] for p in bt])
            k0, k1 = data['mkpts0_f'].cpu().numpy(), data['mkpts1_f'].cpu().numpy()
            sc, bids = data['mconf'].cpu().numpy(), data['m_bids'].cpu().numpy()
            for q in range(len(bt)):
                sel = bids == q
                results.append((np.concatenate([k0[sel], k1[sel]], axis=1), k0[sel], k1[sel], sc[sel]))
    total = sum(len(r[0]) for r in results)
    log(f'load: {len(pairs)} pairs over {K} images of 640 x 640, fp16, batches of {batch}, thresholds 0.2 / 0.1, planted maps: {total} rows '
        f'({total / len(pairs):.0f} per pair); every image SIMPLE_RADIAL 640 640 600 320 320 -0.1')

    res, _ = MT.undistort_results(pairs, results, cams, device=DEV)
    h_res, _ = CC.host_undistorted_results(pairs, results, cams)
    same = all(a[0].tobytes() == b[0].tobytes() for a, b in zip(res, h_res))
    log(f'device result against the host build: {"bit-equal" if same else "DIFFERENT"}; rows without a pre-image: {int(res.n_failed.sum())}')

    rows = torch.from_numpy(np.concatenate([np.asarray(r[0], np.float32) for r in results])).to(DEV)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r[0]) for r in results])]).astype(np.int32)).to(DEV)
    pim = torch.tensor(idx_pairs, dtype=torch.int32, device=DEV).t().contiguous()
    tab = ops.camera_table([MT.canonical_camera(cams[n]) for n in names], DEV)
    out = torch.empty(2, len(rows), 2, dtype=torch.float32, device=DEV)
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    def kernel_form():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for s in (0, 1):
            ops.undistort_points(rows[:, 2 * s:2 * s + 2], off, pim[s], tab, out=out[s], flags=flags)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    forms = {'device': lambda: timed(lambda: MT.undistort_results(pairs, results, cams, device=DEV)), 'kernel': kernel_form,
             'host': lambda: timed(lambda: CC.host_undistorted_results(pairs, results, cams)),
             'consolidate': lambda: timed(lambda: MT.consolidate_matches(pairs, results, device=DEV))}
    for fn in forms.values():
        for _ in range(2):
            fn()
    t = {k: [] for k in forms}
    for _ in range(WINDOWS):
        for k, fn in forms.items():
            t[k].append(fn())
    log(f'{WINDOWS} windows per form, the forms alternating; one window = one pass over the {len(pairs)} pairs')
    log(line('(a) undistort_results end to end', t['device'], 'ms'))
    log(line('(b) the two launches alone (device events)', t['kernel'], 'ms'))
    log(line('(c) host C++ build on the same rows, both sides', t['host'], 'ms'))
    log(line('(d) consolidate_matches on the same tuples, the yardstick', t['consolidate'], 'ms'))
    a, b, c, d = (statistics.median(t[k]) for k in ('device', 'kernel', 'host', 'consolidate'))
    log(f'per row and side: {1e6 * b / (2 * total):.2f} ns in the kernel; undistort_results / consolidate_matches = {a / d:.2f}; device / host = '
        f'{a / c:.2f}')


if __name__ == '__main__':
    main()
