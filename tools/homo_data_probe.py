"""Timing record of the homography-pair generator (geoformer_amd/train/homo_data.py), on the GPU machine:
   python tools/homo_data_probe.py [--out profiles/homo_data.txt]
For generated PPM sources of 480x640 and 768x1024 going to 480x640 (size=(480, 640), st=32):
   * HomoPairs.batch() for a 4-pair batch, preprocess 'host' and 'device': ms per batch and pairs/s, decode included, next to the 0.104 s
     training step of BASELINE configs[2] (the batch this loader has to feed);
   * the kernel alone: gf_image_warp_resize with a perspective matrix between device events, 100 launches per window through the C entry
     itself, with gf_image_gray_resize at the same shapes as the yardstick, and the host's time to ENQUEUE one launch beside it (a window
     cannot be shorter than 100 enqueues: where the two figures meet, the kernel figure is an upper bound).
Every figure is the median (min .. max) of REPEATS timed windows after a warm-up, each window closed by a device synchronise."""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 7
SHAPES = [(480, 640), (768, 1024)]
STEP_S = 0.104                      # BASELINE configs[2]: 640x480, batch 4 per GPU


def _windows(fn, sync, warmup=2, repeats=REPEATS):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def _texture(h, w, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    g = sum(np.sin(xx * fx + yy * fy + p) for fx, fy, p in rng.uniform(0.01, 0.35, (12, 3)))
    rgb = 127 + 18 * g[..., None] + rng.normal(0, 6, (h, w, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8)


def _kernel_us(call, sync):
    """(device time per launch between events, host time to enqueue one launch), microseconds: medians of REPEATS windows of 100 launches."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev, host = [], []
    for _ in range(REPEATS + 2):
        sync()
        e0.record()
        t = time.perf_counter()
        for _ in range(100):
            call()
        host.append((time.perf_counter() - t) * 1e4)
        e1.record()
        e1.synchronize()
        dev.append(e0.elapsed_time(e1) * 10)
    return statistics.median(dev[2:]), min(dev[2:]), max(dev[2:]), statistics.median(host[2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'homo_data.txt'))
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from geoformer_amd import _lib, ops
    from geoformer_amd.train.homo_data import HomoPairs
    dev = 'cuda'
    sync = torch.cuda.synchronize
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)
    say(f'device: {torch.cuda.get_device_name(0)}; median (min .. max) of {REPEATS} windows after a warm-up; target 480x640 fp32, PPM sources')
    say('HomoPairs.batch(), 4 pairs per batch, decode included (one window = one batch):')
    M = np.array([[0.93, 0.06, 21.], [-0.04, 1.05, -13.], [6e-5, -4e-5, 1.]])
    h_lib = _lib.lib()
    for h, w in SHAPES:
        with tempfile.TemporaryDirectory() as tmp:
            for k in range(4):
                Image.fromarray(_texture(h, w, k)).save(os.path.join(tmp, f'{k}.ppm'))
            res = {}
            for pre in ('host', 'device'):
                ds = HomoPairs(tmp, size=(480, 640), st=32, seed=1, device=dev, preprocess=pre)
                assert ds.target_hw(0) == (480, 640)
                res[pre] = (ds, _windows(lambda ds=ds: ds.batch([0, 1, 2, 3]), sync))
            a, b = (res[p][0].batch([0, 1, 2, 3]) for p in ('host', 'device'))
            assert all(torch.equal(a[k], b[k]) for k in ('image0', 'image1', 'H_0to1', 'H_1to0')), 'device path differs from host path'
            for pre, (_, (med, lo, hi)) in res.items():
                say(f'  {h:>4}x{w:<4} preprocess={pre:<6}: {med:8.2f} ms per batch ({lo:.2f} .. {hi:.2f}) = {4e3 / med:7.1f} pairs/s; '
                    f'{med / (STEP_S * 1e3) * 100:6.1f} % of the {STEP_S} s step of configs[2]')
            say(f'  {h:>4}x{w:<4} host / device: {res["host"][1][0] / res["device"][1][0]:.1f} x')
    say('kernel alone, us per launch between device events (100 launches per window) | host time to enqueue one launch:')
    for h, w in SHAPES:
        d_rgb = torch.from_numpy(_texture(h, w, 0)).to(dev)
        out = torch.empty(480, 640, device=dev)
        want = ops.image_warp_resize(d_rgb, M, 640, 480)
        minv = (ctypes.c_double * 9)(*np.linalg.inv(M).reshape(-1))
        bc = (ctypes.c_float * 2)(1.2, 0.0)
        src, dst = ctypes.c_void_p(d_rgb.data_ptr()), ctypes.c_void_p(out.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        calls = {'gf_image_warp_resize': lambda: h_lib.gf_image_warp_resize(src, 3, h, w, 3 * w, minv, h, w, dst, 1, 480, 640, None, stream),
                 'gf_image_warp_resize + brightness/contrast': lambda: h_lib.gf_image_warp_resize(src, 3, h, w, 3 * w, minv, h, w, dst, 1, 480, 640, bc, stream),
                 'gf_image_gray_resize (yardstick)': lambda: h_lib.gf_image_gray_resize(src, 3, h, w, 3 * w, dst, 1, 480, 640, stream)}
        assert calls['gf_image_warp_resize']() == 0
        sync()
        assert torch.equal(out, want[0, 0])
        for name, call in calls.items():
            med, lo, hi, enq = _kernel_us(call, sync)
            say(f'  {h:>4}x{w:<4} {name:<44}: {med:7.2f} ({lo:.2f} .. {hi:.2f}) | {enq:6.2f}')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
