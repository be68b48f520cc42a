"""What consolidating pair matches into keypoints and match ids costs next to the matching it follows, measured in ONE process:
    python tools/keypoint_probe.py [--out profiles/keypoint_quantize.txt]

Load: that of tools/feature_cache_probe.py leg (1) - all 120 pairs of 16 images of 640 x 640 (fp16, batches of 8, thresholds 0.2 / 0.1,
planted maps), matched once outside the timed windows into match_pairs-style tuples; consolidation with the reference's defaults
(sc_thres 0.25, psize 48, dthres 4, unique).  Timed forms, after warm-up, 7 windows per form alternating form by form, reported as median
with min .. max:
  (a) matcher.consolidate_matches end to end: host packing, the one upload, the device path, the reads of the results (host clock);
  (b) the walk kernel alone, between device events around its launch (gf_profile_*, tag kp_walk), inside form (a)'s calls;
  (c) the serial host C++ build (csrc/host/keypoint_host.cpp) on the same tuples, concatenation included (host clock);
  (d) the yardstick: extract_features once per image + match_features for the same 120 pairs (host clock).
Also reported: points, groups, the longest group, the most centres in a group, keypoints per image, rows dropped by the filter, and that
(a) and (c) agree bit for bit."""
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
        raise SystemExit('keypoint_probe: needs an MI355X')
    import bench
    import keypoint_cases as KC
    from feature_cache_probe import planted_images
    from geoformer_amd import _lib, matcher as MT, miopen
    from geoformer_amd.model.full_model import ImageFeatures
    miopen.use_shipped_find_db()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    log(f'keypoint_probe on {torch.cuda.get_device_name(0)}, torch {torch.__version__}')
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
    log(f'load: {len(pairs)} pairs over {K} images of 640 x 640, fp16, batches of {batch}, thresholds 0.2 / 0.1, planted maps: {total} matches '
        f'({total / len(pairs):.0f} per pair); consolidation with sc_thres 0.25, psize 48, dthres 4, unique')

    def host_form():
        im = np.array(idx_pairs, np.int32)
        ms = [np.asarray(r[0], np.float32).reshape(-1, 4) for r in results]
        ss = [np.asarray(r[3], np.float32) for r in results]
        off = np.concatenate([[0], np.cumsum([len(x) for x in ms])]).astype(np.int32)
        return KC.host_consolidate(np.concatenate(ms), np.concatenate(ss), off, im, K)

    kp, kpo, ids, ido, st = host_form()
    cm = MT.consolidate_matches(pairs, results, device=DEV)
    same = (all(np.array_equal(cm.keypoints[i].view(np.uint32), kp[kpo[i]:kpo[i + 1]].view(np.uint32)) for i in range(K))
            and all(np.array_equal(cm.matches[q], ids[ido[q]:ido[q + 1]]) for q in range(len(pairs))))
    log(f'device result against the host build: {"bit-equal (keypoints, ids, order)" if same else "DIFFERENT"}')
    log(f'points {st["points"]} (2 x {st["points"] // 2} rows at or above the threshold of {total}), groups {st["groups"]}, longest group '
        f'{st["longest_group"]} points, most centres in a group {st["most_centres"]}, keypoints {st["K"]} '
        f'(per image {int(np.diff(kpo).min())} .. {int(np.diff(kpo).max())}), rows dropped by the filter {st["dropped"]}, rows kept {st["rows"]}')

    h = _lib.lib()
    walk_us = []

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)

    def device_form():
        h.gf_profile_filter(b'kp_walk')
        h.gf_profile_enable(1)
        ms = timed(lambda: MT.consolidate_matches(pairs, results, device=DEV))
        tot, cnt, work = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        h.gf_profile_collect(b'kp_walk', ctypes.byref(tot), ctypes.byref(cnt), ctypes.byref(work))
        h.gf_profile_enable(0)
        h.gf_profile_filter(None)
        walk_us.append(1e3 * tot.value / max(cnt.value, 1))
        return ms

    def plain_device_form():
        return timed(lambda: MT.consolidate_matches(pairs, results, device=DEV))

    def match_form():
        with torch.no_grad():
            return timed(match_pass)

    forms = {'device': device_form, 'device_plain': plain_device_form, 'host': lambda: timed(host_form), 'match': match_form}
    for fn in forms.values():
        for _ in range(2):
            fn()
    walk_us.clear()
    out = {k: [] for k in forms}
    for _ in range(WINDOWS):
        for k, fn in forms.items():
            out[k].append(fn())
    log(f'{WINDOWS} windows per form, the forms alternating; one window = one pass over the {len(pairs)} pairs')
    log(line('(a) consolidate_matches end to end, walk kernel under events', out['device'], 'ms'))
    log(line('(a) consolidate_matches end to end, no events', out['device_plain'], 'ms'))
    log(line('(b) walk kernel alone (device events)', [u / 1e3 for u in walk_us], 'ms'))
    log(line('(c) host C++ build on the same tuples', out['host'], 'ms'))
    log(line('(d) extract_features + match_features, the 120 pairs', out['match'], 'ms'))
    a, c, d = (statistics.median(out[k]) for k in ('device_plain', 'host', 'match'))
    log(f'per pair: consolidation {1e3 * a / len(pairs):.1f} us on the device path, {1e3 * c / len(pairs):.1f} us on the host build; matching '
        f'{1e3 * d / len(pairs):.1f} us.  device / host = {a / c:.2f}; consolidation / matching = {a / d:.3f} (device), {c / d:.3f} (host)')


if __name__ == '__main__':
    main()
