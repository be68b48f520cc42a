"""Host vs device image preprocessing of the matcher (load_gray_scale_tensor preprocess='host' | 'device'), on the GPU machine:
   python tools/preprocess_probe.py                 every step below, each in a child process of its own under a time limit
   python tools/preprocess_probe.py --step images   ms per image for four source shapes -> 480x640 (imsize 480, shorter side, x8):
                                                    numpy gray + resize + upload against pinned upload + one kernel, decode excluded
                                                    and included, plus the kernel alone between device events
   python tools/preprocess_probe.py --step pairs --precision fp16|bf16
                                                    match_pairs pairs/s for both settings on synthetic PPM files in a temporary directory
Every figure is the median of REPEATS timed windows after a warm-up, each window closed by a device synchronise."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 7
SHAPES = [(600, 800), (768, 1024), (1200, 1600), (480, 640)]


def _median_ms(fn, sync, warmup=3, repeats=REPEATS, inner=1):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        ts.append((time.perf_counter() - t) * 1e3 / inner)
    return statistics.median(ts), min(ts), max(ts)


def _texture(h, w, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    g = sum(np.sin(xx * fx + yy * fy + p) for fx, fy, p in rng.uniform(0.01, 0.35, (12, 3)))
    rgb = 127 + 18 * g[..., None] + rng.normal(0, 6, (h, w, 3))
    return np.clip(rgb, 0, 255).astype(np.uint8)


def step_images():
    import numpy as np
    import torch
    from PIL import Image
    from geoformer_amd import matcher as MT, ops
    dev = 'cuda'
    sync = torch.cuda.synchronize
    print(f'device: {torch.cuda.get_device_name(0)}; median (min .. max) of {REPEATS} windows, ms per image, target 480x640 fp32')
    print(f'{"source":>10} | {"host: gray+resize+upload":>26} | {"device: upload+kernel":>24} | {"kernel alone":>12} | '
          f'{"host incl. decode":>20} | {"device incl. decode":>20}')
    worse = []
    with tempfile.TemporaryDirectory() as tmp:
        for h, w in SHAPES:
            rgb = np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)
            path = os.path.join(tmp, f'{h}x{w}.ppm')
            Image.fromarray(rgb).save(path)
            wt, ht, _ = MT.resize_im(w, h, imsize=480, dfactor=8, value_to_scale=min)

            def host():
                im = MT.cv2_resize_linear_u8(MT.cv2_gray_u8(rgb), wt, ht)
                return torch.from_numpy(im).to(device=dev, dtype=torch.float32)[None, None] / 255.0

            def device():
                return ops.image_gray_resize(MT._staging.upload(rgb, dev, 0), wt, ht, reciprocal=True)       # as load_gray_scale_tensor does
            assert torch.equal(host().view(torch.int32), device().view(torch.int32)), 'device path differs from host path'
            d_rgb = torch.from_numpy(rgb).to(dev)
            out = torch.empty(ht, wt, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            kern = []
            for _ in range(REPEATS + 2):
                e0.record()
                for _ in range(100):
                    ops.image_gray_resize(d_rgb, wt, ht, out=out)
                e1.record()
                e1.synchronize()
                kern.append(e0.elapsed_time(e1) / 100)
            th = _median_ms(host, sync)
            td = _median_ms(device, sync)
            thd = _median_ms(lambda: MT.load_gray_scale_tensor(path, dev, imsize=480, preprocess='host'), sync)
            tdd = _median_ms(lambda: MT.load_gray_scale_tensor(path, dev, imsize=480, preprocess='device'), sync)
            fmt = lambda t: f'{t[0]:7.3f} ({t[1]:.3f} .. {t[2]:.3f})'
            print(f'{h:>5}x{w:<4} | {fmt(th):>26} | {fmt(td):>24} | {statistics.median(kern[2:]):>12.4f} | {fmt(thd):>20} | {fmt(tdd):>20}', flush=True)
            if not (td[0] < th[0] and tdd[0] < thd[0]):
                worse.append((h, w))
    print('device path below host path for every probed shape: ' + ('yes' if not worse else f'NO, not for {worse}'))


def step_pairs(precision):
    import torch
    from PIL import Image
    from geoformer_amd import matcher as MT
    from geoformer_amd.weights import deterministic_init_
    sync = torch.cuda.synchronize
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for k, (h, w) in enumerate([(768, 1024), (600, 800)]):
            files.append(os.path.join(tmp, f'{k}.ppm'))
            Image.fromarray(_texture(h, w, k)).save(files[-1])
        ms = {}
        for pre in MT.PREPROCESS:
            ms[pre] = MT.GeoFormerMatcher(imsize=480, match_threshold=0.2, no_match_upscale=True, precision=precision, preprocess=pre)
            deterministic_init_(ms[pre].model)
        n = {pre: len(m.match_pairs(*files)[0]) for pre, m in ms.items()}
        res = {pre: _median_ms(lambda m=m: m.match_pairs(*files), sync, warmup=5, inner=20) for pre, m in ms.items()}
        for pre, (med, lo, hi) in res.items():
            print(f'match_pairs {precision} preprocess={pre:<6}: {1e3 / med:7.1f} pairs/s  ({med:.2f} ms/pair, windows {lo:.2f} .. {hi:.2f}; '
                  f'{n[pre]} matches, 768x1024 + 600x800 PPM -> 480x640)', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', choices=('images', 'pairs'), default=None)
    ap.add_argument('--precision', choices=('fp16', 'bf16'), default='fp16')
    ap.add_argument('--timeout', type=int, default=300, help='seconds per step')
    args = ap.parse_args()
    if args.step == 'images':
        return step_images()
    if args.step == 'pairs':
        return step_pairs(args.precision)
    for extra in (['--step', 'images'], ['--step', 'pairs', '--precision', 'fp16'], ['--step', 'pairs', '--precision', 'bf16']):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *extra], timeout=args.timeout)
        if r.returncode != 0:                     # nothing more is started on the device after a failed step
            sys.exit(f'step {extra} failed with status {r.returncode}')


if __name__ == '__main__':
    main()
