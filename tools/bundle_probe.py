"""What bundle adjustment costs, measured in ONE process:
    python tools/bundle_probe.py [--out profiles/bundle_adjust.txt]
A record, not a gate.

Load 1: the triangulation probe's database (tools/triangulate_probe.py: 16 images on an arc, all 120 pairs, 12,000 planted points of which
every image sees 39 %, 0.5 px noise, 1 % mismatched rows), the poses of 14 images perturbed by 1 degree and 0.05 units and free, the two
end images fixed; triangulated at 20 px from the rough poses, then matcher.refine with thr 20 px and 16 iterations.
Load 2: 130 cameras on an arc (tests/bundle_cases.py), 3,000 points of which a camera sees a tenth, 128 cameras free, 16 iterations, through
ops.bundle_adjust: what the one-workgroup Cholesky of the 768 x 768 reduced system costs.
Timed forms, after warm-up, 7 windows per form alternating form by form, median with min .. max:
  (a) matcher.refine (load 1) / ops.bundle_adjust (load 2) end to end, host clock, no events;
  (b) .. (e) the kernels between device events, summed over the 16 iterations of one call (gf_profile_*, tags ba_points, ba_camera_rows,
      ba_cholesky, ba_update_cost = ba_update + ba_cost + ba_decide), each inside form (a)'s call;
  (f) the serial host build (csrc/host/ba_host.cpp) on the same input (host clock, 3 runs).
The PCG section (--section pcg, or all): loads 1 and 2 again with solver='pcg' beside the dense solver - end to end, in the same process,
the windows alternating dense, pcg, dense, .. -, then the kernels of the PCG call between device events (tags ba_points, ba_pcg_setup,
ba_pcg_points, ba_pcg_cameras, ba_pcg_step, ba_update_cost), cg_used per iteration, and the serial host build of the PCG rule.
Load 3: 1,002 cameras on the arc, 3,000 points of which a camera sees three in a hundred, 1,000 cameras free - more than the dense
solver takes -, 16 iterations, solver='pcg' only."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = 'cuda:0'
WINDOWS = 7
TAGS = (b'ba_points', b'ba_camera_rows', b'ba_cholesky', b'ba_update_cost')
PCG_TAGS = (b'ba_points', b'ba_pcg_setup', b'ba_pcg_points', b'ba_pcg_cameras', b'ba_pcg_step', b'ba_update_cost')


def line(name, v, unit):
    return f'  {name:<66s} {statistics.median(v):10.3f} {unit}  (min {min(v):.3f} .. max {max(v):.3f})'


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def side_by_side(log, dense, pcg, label):
    """end to end, the windows alternating dense, pcg, dense, .."""
    for fn in (dense, pcg):
        for _ in range(2):
            timed(fn)
    out = {'dense': [], 'pcg': []}
    for _ in range(WINDOWS):
        out['dense'].append(timed(dense))
        out['pcg'].append(timed(pcg))
    log(f'{label}: end to end, {WINDOWS} windows per solver, alternating')
    log(line("solver='dense'", out['dense'], 'ms'))
    log(line("solver='pcg'", out['pcg'], 'ms'))


def measure(log, h, run, host_run, label, TAGS=TAGS):
    kern = {tag: [] for tag in TAGS}

    def under_events(tag):
        h.gf_profile_filter(tag)
        h.gf_profile_enable(1)
        ms = timed(run)
        tot, cnt, work = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        h.gf_profile_collect(tag, ctypes.byref(tot), ctypes.byref(cnt), ctypes.byref(work))
        h.gf_profile_enable(0)
        h.gf_profile_filter(None)
        kern[tag].append(tot.value)
        return ms

    forms = {'e2e': lambda: timed(run), **{tag: (lambda tag=tag: under_events(tag)) for tag in TAGS}}
    for fn in forms.values():
        for _ in range(2):
            fn()
    for v in kern.values():
        v.clear()
    out = {k: [] for k in forms}
    for _ in range(WINDOWS):
        for k, fn in forms.items():
            out[k].append(fn())
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        host_run()
        host_ms.append(1e3 * (time.perf_counter() - t0))
    log(f'{label}: {WINDOWS} windows per form, the forms alternating; one window = one call of 16 iterations')
    log(line('(a) end to end, no events', out['e2e'], 'ms'))
    for name, tag in zip('bcdeghi', TAGS):
        log(line(f'({name}) {tag.decode()} (device events, 16 iterations summed)', kern[tag], 'ms'))
    log(line('(f) serial host build, the same input (3 runs)', host_ms, 'ms'))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    ap.add_argument('--section', choices=('all', 'dense', 'pcg'), default='all', help='which part of the record to measure')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bundle_probe: needs an MI355X')
    import bundle_cases as bc
    import bundle_pcg_cases as pc
    import triangulate_probe as TP
    from geoformer_amd import _lib, matcher as MT, ops
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    log(f'bundle_probe on {torch.cuda.get_device_name(0)}, torch {torch.__version__}')
    h = _lib.lib()
    ITERS, THR = 16, 20.0

    # load 1
    cm, intr, poses = TP.planted_matches(16, 12000, 0.39, 0.8, 0.01, 2025)
    rng = np.random.default_rng(3)
    fixed = [cm.names[0], cm.names[-1]]
    rough = {}
    for nm, (R, t) in poses.items():
        if nm in fixed:
            rough[nm] = (R, t)
            continue
        w, d = rng.normal(size=3), rng.normal(size=3)
        Rn = bc.rodrigues(w * np.deg2rad(1.0) / np.linalg.norm(w)) @ R
        rough[nm] = (Rn, -Rn @ (-R.T @ t + 0.05 * d / np.linalg.norm(d)))
    tt = MT.triangulate(cm, intr, rough, thr=THR, device=DEV)
    rs = MT.refine(cm, tt, intr, rough, fixed=fixed, iters=ITERS, thr=THR, device=DEV)
    a = MT._refine_inputs(cm, tt, intr, rough, fixed)
    ref = bc.host_refine_device(a, (THR,), ITERS)
    dev = MT._refine_device(a, (THR,), ITERS, DEV)
    same = all(np.asarray(dev[k]).tobytes() == np.asarray(ref[k]).tobytes() for k in ('R', 't', 'X', 'cost', 'accepted', 'inliers'))
    cen = lambda P: np.array([np.linalg.norm(-P[nm][0].T @ P[nm][1] + poses[nm][0].T @ poses[nm][1]) for nm in cm.names if nm not in fixed])
    log(f'load 1: {len(cm.names)} images ({rs.n_free} free), {len(tt.points)} points, {len(tt.obs_image)} observations, thr {THR} px, {ITERS} '
        f'iterations: {int(rs.accepted.sum())} accepted, cost {rs.cost[0]:.6g} -> {rs.cost[-1]:.6g}, median centre error of the free cameras '
        f'{np.median(cen(rough)):.5f} -> {np.median(cen(rs.poses)):.5f}; {len(rs.tracks.points)} points kept; device == host build: {same}')
    if args.section != 'pcg':
        measure(log, h, lambda: MT.refine(cm, tt, intr, rough, fixed=fixed, iters=ITERS, thr=THR, device=DEV),
                lambda: bc.host_refine_device(a, (THR,), ITERS), 'load 1')
    if args.section != 'dense':
        rp = MT.refine(cm, tt, intr, rough, fixed=fixed, iters=ITERS, thr=THR, device=DEV, solver='pcg')
        ref = pc.host_refine_device_pcg(a, (THR,), ITERS, solver='pcg')
        dev = MT._refine_device(a, (THR,), ITERS, DEV, solver='pcg')
        same = all(np.asarray(dev[k]).tobytes() == np.asarray(ref[k]).tobytes() for k in ('R', 't', 'X', 'cost', 'accepted', 'inliers', 'cg_used'))
        log(f"load 1, solver='pcg' (cg_iters 64, cg_tol 1e-6): {int(rp.accepted.sum())} accepted, cost {rp.cost[0]:.6g} -> {rp.cost[-1]:.6g}, median "
            f'centre error of the free cameras {np.median(cen(rough)):.5f} -> {np.median(cen(rp.poses)):.5f}; cg_used {rp.cg_used.tolist()}; device == '
            f'host build: {same}')
        side_by_side(log, lambda: MT.refine(cm, tt, intr, rough, fixed=fixed, iters=ITERS, thr=THR, device=DEV),
                     lambda: MT.refine(cm, tt, intr, rough, fixed=fixed, iters=ITERS, thr=THR, device=DEV, solver='pcg'), 'load 1')
        measure(log, h, lambda: MT.refine(cm, tt, intr, rough, fixed=fixed, iters=ITERS, thr=THR, device=DEV, solver='pcg'),
                lambda: pc.host_refine_device_pcg(a, (THR,), ITERS, solver='pcg'), "load 1, solver='pcg'", PCG_TAGS)

    # load 2
    s = bc.make_scene(5, n_cams=130, n_points=3000, drop=0.9)
    free = bc.free_flags(s)
    bc.keep_fixed_true(s, free)
    d = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=DEV)
    td = [d(s.obs_off, torch.int32), d(s.obs_image, torch.int32), d(s.uv, torch.float32), d(s.K, torch.float32), d(s.R, torch.float64),
          d(s.t, torch.float64), d(s.X, torch.float64), d(free, torch.bool)]
    host = {'obs_off': s.obs_off, 'obs_image': s.obs_image, 'free': free}
    run2 = lambda: ops.bundle_adjust(*td, thr=THR, iters=ITERS, host=host)
    o = {k: v.cpu().numpy() for k, v in run2().items()}
    ref = bc.run_host_scene(s, free, THR, ITERS)
    same = all(np.asarray(o[k]).tobytes() == np.asarray(ref[k]).tobytes() for k in ('R', 't', 'X', 'cost', 'accepted', 'lam', 'inliers', 'status'))
    log(f'load 2: {len(s.K)} images ({int(free.sum())} free: a {6 * int(free.sum())} x {6 * int(free.sum())} reduced system), {len(s.X)} points, '
        f'{len(s.uv)} observations, thr {THR} px, {ITERS} iterations: {int(o["accepted"].sum())} accepted, cost {o["cost"][0]:.6g} -> '
        f'{o["cost"][-1]:.6g}, median centre error of the free cameras {np.median(bc.centre_errors(s.R, s.t, s)[free]):.5f} -> '
        f'{np.median(bc.centre_errors(o["R"], o["t"], s)[free]):.5f}; device == host build: {same}')
    if args.section != 'pcg':
        measure(log, h, run2, lambda: bc.run_host_scene(s, free, THR, ITERS), 'load 2')
    if args.section == 'dense':
        return

    def pcg_load(s, free, td, host, label):
        run = lambda: ops.bundle_adjust(*td, thr=THR, iters=ITERS, host=host, solver='pcg')
        o = {k: v.cpu().numpy() for k, v in run().items()}
        ref = pc.run_host_pcg_scene(s, free, THR, ITERS)
        same = all(np.asarray(o[k]).tobytes() == np.asarray(ref[k]).tobytes() for k in o)
        log(f"{label}, solver='pcg' (cg_iters 64, cg_tol 1e-6): {len(s.K)} images ({int(free.sum())} free), {len(s.X)} points, {len(s.uv)} "
            f'observations, thr {THR} px, {ITERS} iterations: {int(o["accepted"].sum())} accepted, cost {o["cost"][0]:.6g} -> {o["cost"][-1]:.6g}, '
            f'median centre error of the free cameras {np.median(bc.centre_errors(s.R, s.t, s)[free]):.5f} -> '
            f'{np.median(bc.centre_errors(o["R"], o["t"], s)[free]):.5f}; cg_used {o["cg_used"].tolist()}; device == host build: {same}')
        return run
    run2p = pcg_load(s, free, td, host, 'load 2')
    side_by_side(log, run2, run2p, 'load 2')
    measure(log, h, run2p, lambda: pc.run_host_pcg_scene(s, free, THR, ITERS), "load 2, solver='pcg'", PCG_TAGS)

    # load 3: beyond the dense solver
    s = bc.make_scene(6, n_cams=1002, n_points=3000, drop=0.97)
    free = bc.free_flags(s)
    bc.keep_fixed_true(s, free)
    td = [d(s.obs_off, torch.int32), d(s.obs_image, torch.int32), d(s.uv, torch.float32), d(s.K, torch.float32), d(s.R, torch.float64),
          d(s.t, torch.float64), d(s.X, torch.float64), d(free, torch.bool)]
    host = {'obs_off': s.obs_off, 'obs_image': s.obs_image, 'free': free}
    run3 = pcg_load(s, free, td, host, 'load 3')
    measure(log, h, run3, lambda: pc.run_host_pcg_scene(s, free, THR, ITERS), "load 3, solver='pcg'", PCG_TAGS)


if __name__ == '__main__':
    main()
