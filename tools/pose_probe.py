"""Timing record of the device relative-pose path at the benchmark's load: 8 pairs x ~2300 matches, 1024 hypotheses per pair.

    python tools/pose_probe.py [--out profiles/pose_ransac.txt] [--matches 2300] [--iters 1024]

Three steps, each a fresh child process under its own time limit; the first failure stops the script:
    pose        ops.ransac_essential   (pose_score + pose_final)
    epipolar    ops.epipolar_errors
    homography  ops.ransac_homography (gf_ransac_homography_v2) on the same matches: the yardstick - there is no parent to compare with
Per step: 10 warm-up calls, then 7 windows of 200 calls, each window between device synchronisations (host clock); the record is the
median window and the spread (min .. max).  What is timed is the OP CALL - the Python wrapper (output allocations, workspace lookup), the
launches and the kernels - not kernel time: for the small epipolar kernel that is mostly host enqueue cost.  A record, not a gate.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {'pose': 240, 'epipolar': 180, 'homography': 180}          # time limit of the child, seconds (torch import + scene + ~2 s of timing)


F, CX, CY = 500.0, 320.0, 240.0


def _scene(rng, n, outlier_frac=0.3, noise_px=0.25):
    """A planted two-view scene (the generator of the pose tests, vectorised): 12-degree rotations, unit baselines, points 4 .. 10 in front
    of camera 0, 640 x 480 images at f = 500; outliers are uniform second-image points at least 10 px (Sampson) from the truth."""
    import numpy as np
    v = rng.standard_normal(3) * np.deg2rad(12.0)
    th = np.linalg.norm(v)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.standard_normal(3)
    t /= np.linalg.norm(t)
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    X = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2, 2, n), rng.uniform(4, 10, n)], 1)
    Y = X @ R.T + t
    x0, x1 = X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]
    x1 = x1 + rng.standard_normal((n, 2)) * noise_px / F
    todo = np.flatnonzero(rng.random(n) < outlier_frac)
    h0 = np.c_[x0, np.ones(n)]
    for _ in range(50):                                # bounded: a keypoint on the epipole has no point 10 px from its "line" and stays an inlier
        if not len(todo):
            break
        q = np.c_[(rng.uniform(0, 640, len(todo)) - CX) / F, (rng.uniform(0, 480, len(todo)) - CY) / F, np.ones(len(todo))]
        a, b = h0[todo] @ E.T, q @ E
        d = np.abs(np.sum(q * a, 1)) / np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2) * F
        x1[todo[d > 10.0]] = q[d > 10.0, :2]
        todo = todo[d <= 10.0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    px = lambda x: (x * F + np.array([CX, CY])).astype(np.float32)
    return {'mk0': px(x0), 'mk1': px(x1), 'R': R, 't': t, 'T_0to1': T}


def _pose_err_deg(R, t, R_gt, t_gt):
    import numpy as np
    te = np.degrees(np.arccos(np.clip(np.dot(t, t_gt) / (np.linalg.norm(t) * np.linalg.norm(t_gt)), -1, 1)))
    re = np.degrees(np.arccos(np.clip((np.trace(R.T @ R_gt) - 1) / 2, -1, 1)))
    return max(re, min(te, 180 - te))


def load(n_pairs, n_matches):
    import numpy as np
    rng = np.random.default_rng(900)
    scenes = [_scene(rng, n_matches) for _ in range(n_pairs)]
    return scenes, np.concatenate([s['mk0'] for s in scenes]), np.concatenate([s['mk1'] for s in scenes])


def child(step, n_pairs, n_matches, iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from geoformer_amd import ops
    assert torch.cuda.is_available(), 'the probe measures on the GPU only'
    scenes, mk0, mk1 = load(n_pairs, n_matches)
    dev = 'cuda'
    mk0, mk1 = torch.tensor(mk0, device=dev), torch.tensor(mk1, device=dev)
    counts = torch.tensor([n_pairs * n_matches] + [n_matches] * n_pairs, dtype=torch.int32, device=dev)
    K = torch.tensor([[[F, 0, CX], [0, F, CY], [0, 0, 1]]] * n_pairs, dtype=torch.float32, device=dev)
    bids = torch.arange(n_pairs, device=dev).repeat_interleave(n_matches)
    T = torch.tensor(np.stack([s['T_0to1'] for s in scenes]), dtype=torch.float32, device=dev)
    if step == 'pose':
        call = lambda: ops.ransac_essential(mk0, mk1, counts, n_pairs, K, K, pixel_thr=0.5, iters=iters)
    elif step == 'epipolar':
        call = lambda: ops.epipolar_errors(mk0, mk1, bids, T, K, K)
    else:
        call = lambda: ops.ransac_homography(mk0, mk1, counts, n_pairs, 1.0, thr=3.0, iters=iters, integer_keypoints=False, min_points=4)
    for _ in range(10):
        out = call()
    torch.cuda.synchronize()
    windows = []
    for _ in range(7):
        t = time.perf_counter()
        for _ in range(200):
            out = call()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t) / 200 * 1e6)
    rec = {'step': step, 'us_median': float(np.median(windows)), 'us_min': min(windows), 'us_max': max(windows)}
    if step == 'pose':
        R, t = out['R'].cpu().numpy(), out['t'].cpu().numpy()
        errs = [_pose_err_deg(R[i], t[i], s['R'], s['t']) for i, s in enumerate(scenes)]
        rec.update(valid=out['valid'].tolist(), n_inliers=out['n_inliers'].tolist(), worst_pose_err_deg=float(max(errs)))
    elif step == 'homography':
        rec.update(valid=out['valid'].tolist())
    print('POSE_PROBE ' + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', choices=list(STEPS))
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--matches', type=int, default=2300)
    ap.add_argument('--iters', type=int, default=1024)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pose_ransac.txt'))
    a = ap.parse_args()
    if a.step:
        return child(a.step, a.pairs, a.matches, a.iters)
    lines = [f'tools/pose_probe.py: {a.pairs} pairs x {a.matches} matches (30 % outliers, 0.25 px noise), {a.iters} hypotheses per pair; '
             'op call time (wrapper + launches + kernels) in us, median of 7 windows of 200 calls (min .. max)']
    for step, limit in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), '--step', step, '--pairs', str(a.pairs), '--matches', str(a.matches), '--iters', str(a.iters)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired as e:
            sys.exit(f'step {step} exceeded its {limit} s limit: stopping\n{(e.stdout or b"")[-2000:]}\n{(e.stderr or b"")[-2000:]}')
        rec = [l for l in r.stdout.splitlines() if l.startswith('POSE_PROBE ')]
        if r.returncode != 0 or not rec:
            sys.exit(f'step {step} failed ({r.returncode}): stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
        d = json.loads(rec[-1][len('POSE_PROBE '):])
        extra = {k: v for k, v in d.items() if k not in ('step', 'us_median', 'us_min', 'us_max')}
        lines.append(f'{step:11s} {d["us_median"]:9.1f} us  ({d["us_min"]:.1f} .. {d["us_max"]:.1f})  {json.dumps(extra) if extra else ""}')
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
