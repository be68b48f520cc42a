"""What keeping an image's backbone features buys, and what the address-table kernels cost, measured in ONE process so that the
forms compared share the machine's state:   python tools/feature_cache_probe.py [--out profiles/feature_cache.txt] [--legs ...]

  (1) all pairs of 16 images (640 x 640, fp16, 120 pairs in batches of 8, thresholds 0.2 / 0.1 and planted correspondences as bench.py's
      default load): pairs/s through GeoFormer.extract_features (ONE pass over the 16 images, inside the timed window) +
      GeoFormer.match_features, against bench.planted_step - the backbone on the 16 images of every batch of 8 pairs, then
      forward_features - on the same pair batches.  The second form is unchanged code: the yardstick.
  (2) the two address-table kernels at the nominal loads of profiles/mixed_precision.txt against their siblings on stacked maps:
      gf_pos_encode on [16, 256, 80, 80], gf_fine_gather on 36800 windows of 25 x 128; and the torch.stack the table makes unnecessary.
  (3) one query against 50 candidates (640 x 640, fp16, batches of 10): match_features with the query's record named ten times per batch
      (51 extractions inside the window) against planted_step on the 50 pairs.
  (4) is an image's feature record the same at batch 1 and inside a batch of 4?  torch.equal of the backbone's two maps, fp16 and bf16,
      160 x 184 and 640 x 640.  Not a gate: the store keeps whatever `extract` produced.

Method: every form is warmed up; then 7 windows per form, the forms alternating window by window, so a drift of the machine hits all of
them.  Kernel windows are 100 back-to-back launches between two device events; pairs/s windows are a host clock around whole passes
that end in the forward's own host synchronisation, closed by a device synchronise.  Reported: median, minimum and maximum over the
windows - the spread is the yardstick for a difference between two forms.

Planted maps (legs 1 and 3): image k's maps are crops of one random map shifted by k % 9 coarse cells plus noise, so that any two images
correspond by a translation (bench.planted_features' construction for more than two images); every map the matching path reads is
`planted + 0 * backbone output` in an allocation of its own: the planted values bit for bit, the backbone's data dependency kept."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

DEV = 'cuda:0'
F16, BF16 = torch.float16, torch.bfloat16
WINDOWS = 7


def alternate(forms, windows=WINDOWS, warmup=2):
    """forms: {name: fn() -> one window's figure}.  Warm-up windows first, then `windows` rounds with the forms one after the other."""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in forms}
    for _ in range(windows):
        for k, fn in forms.items():
            out[k].append(fn())
    return out


def kernel_window(fn, launches=100):
    def window():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / launches
    return window


def rate_window(fn, pairs, passes):
    def window():
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(passes):
            fn()
        torch.cuda.synchronize()
        return pairs * passes / (time.perf_counter() - t)
    return window


def stat(name, v, unit):
    med = statistics.median(v)
    return f'  {name:<58s} {med:9.1f} {unit}  (min {min(v):.1f}, max {max(v):.1f}, spread {100 * (max(v) - min(v)) / med:.1f} %)'


def verdict(log, what, slow, fast, higher_is_better):
    """Is the difference of two forms' medians larger than their own min - max spreads?"""
    a, b = statistics.median(slow), statistics.median(fast)
    spread = max(max(slow) - min(slow), max(fast) - min(fast))
    ratio = b / a if higher_is_better else a / b
    log(f'  {what}: ratio of the medians {ratio:.3f} x; difference {abs(b - a):.1f} against the larger of the two min - max spreads {spread:.1f}: '
        f'{"OUTSIDE" if abs(b - a) > spread else "inside"} the spread')
    return ratio


# ------------------------------------------------------------------------------------------------------------------------------
def kernel_leg(log):
    from geoformer_amd import ops
    g = torch.Generator().manual_seed(2)
    N, C, H, W = 16, 256, 80, 80
    maps = [(torch.randn(H, W, C, generator=g)).to(DEV, F16).permute(2, 0, 1) for _ in range(N)]          # 16 allocations
    pe = torch.randn(H, W, C, generator=g).to(DEV)
    out = torch.empty(N, H * W, C, dtype=F16, device=DEV)

    def stack(ms):
        return torch.stack([m.permute(1, 2, 0) for m in ms]).permute(0, 3, 1, 2)          # channels-last batch, as the backbone emits
    stacked, batch = stack(maps), ops.MapBatch(maps)
    batch.table()
    assert torch.equal(ops.pos_encode(batch, pe, F16), ops.pos_encode(stacked, pe, F16))
    us = alternate({'tensor': kernel_window(lambda: ops.pos_encode(stacked, pe, F16, out)),
                    'table': kernel_window(lambda: ops.pos_encode(batch, pe, F16, out)),
                    'stack': kernel_window(lambda: stack(maps))})
    log(f'(2a) gf_pos_encode, [{N}, {C}, {H}, {W}] channels-last fp16 -> fp16; {WINDOWS} windows of 100 launches per form, alternating')
    log(stat('gf_pos_encode on the stacked maps', us['tensor'], 'us'))
    log(stat(f'gf_pos_encode_ptrs on {N} separate maps', us['table'], 'us'))
    log(stat(f'torch.stack of the {N} maps (what the table makes unnecessary)', us['stack'], 'us'))
    verdict(log, 'table entry against tensor entry (us; ratio = tensor / table)', us['tensor'], us['table'], False)

    Nf, Cf, CC, hc, M = 8, 128, 256, 80, 8 * 2300
    f0 = [torch.randn(4 * hc, 4 * hc, Cf, generator=g).to(DEV, F16).permute(2, 0, 1) for _ in range(Nf)]
    f1 = [torch.randn(4 * hc, 4 * hc, Cf, generator=g).to(DEV, F16).permute(2, 0, 1) for _ in range(Nf)]
    c0, c1 = (torch.randn(Nf, hc * hc, CC, generator=g).to(DEV, F16) for _ in range(2))
    b = torch.arange(Nf).repeat_interleave(M // Nf).to(DEV)
    i, j = (torch.randint(0, hc * hc, (M,), generator=g).to(DEV) for _ in range(2))
    s0, s1, b0, b1 = stack(f0), stack(f1), ops.MapBatch(f0), ops.MapBatch(f1)
    b0.table(), b1.table()
    args = (c0, c1, b, i, j, hc, hc, 4, 5, F16)
    assert all(torch.equal(x, y) for x, y in zip(ops.fine_gather(b0, b1, *args), ops.fine_gather(s0, s1, *args)))
    us = alternate({'tensor': kernel_window(lambda: ops.fine_gather(s0, s1, *args)),
                    'table': kernel_window(lambda: ops.fine_gather(b0, b1, *args)),
                    'stack': kernel_window(lambda: (stack(f0), stack(f1)))})
    log(f'(2b) gf_fine_gather, {Nf} pairs x {M // Nf} matches = {2 * M} windows of 25 x {Cf}, coarse rows of {CC}, fp16 -> fp16 (one wave per window); '
        f'{WINDOWS} windows of 100 launches per form, alternating')
    log(stat('gf_fine_gather on the stacked maps', us['tensor'], 'us'))
    log(stat(f'gf_fine_gather_ptrs on 2 x {Nf} separate maps', us['table'], 'us'))
    log(stat(f'torch.stack of the 2 x {Nf} fine maps (what the tables make unnecessary)', us['stack'], 'us'))
    verdict(log, 'table entry against tensor entry (us; ratio = tensor / table)', us['tensor'], us['table'], False)


# ------------------------------------------------------------------------------------------------------------------------------
def planted_images(count, seed=60000, grid=80, noise=0.25):
    """-> (coarse [count,256,grid,grid], fine [count,128,4 grid,4 grid]) fp16 channels-last on the device: image k = the common random
    map shifted by k % 9 cells, plus noise (0.25 per image: 0.35 between the two images of a pair, bench.py's figure)."""
    g = torch.Generator().manual_seed(seed)
    big = torch.randn(256, grid + 8, grid + 8, generator=g) * 0.5
    bigf = torch.randn(128, 4 * (grid + 8), 4 * (grid + 8), generator=g)
    cs, fs = [], []
    for k in range(count):
        s = k % 9
        cs.append((big[:, s:s + grid, s:s + grid] + noise * torch.randn(256, grid, grid, generator=g)).to(F16))
        fs.append((bigf[:, 4 * s:4 * (s + grid), 4 * s:4 * (s + grid)] + noise * torch.randn(128, 4 * grid, 4 * grid, generator=g)).to(F16))
    cl = torch.channels_last
    return torch.stack(cs).to(DEV).contiguous(memory_format=cl), torch.stack(fs).to(DEV).contiguous(memory_format=cl)


def pairs_leg(log, tag, model, images, pc, pf, pairs, batch, passes):
    """pairs: [(i, j)] over images [K,1,640,640] with planted maps pc / pf [K, ...].  Both forms walk the same batches of `batch` pairs."""
    import bench
    from geoformer_amd.model.full_model import ImageFeatures
    K = images.shape[0]
    batches = [pairs[s:s + batch] for s in range(0, len(pairs), batch)]
    # the forward form's inputs, gathered per batch OUTSIDE the timed window (a caller of forward has its pair batches already)
    fwd = []
    for bt in batches:
        i0, i1 = torch.tensor([p[0] for p in bt], device=DEV), torch.tensor([p[1] for p in bt], device=DEV)
        idx = torch.cat([i0, i1])
        fwd.append((images[i0], images[i1], {'c': pc[idx].contiguous(memory_format=torch.channels_last),
                                             'f': pf[idx].contiguous(memory_format=torch.channels_last)}))
    chunk = 2 * batch                                  # images per extraction call: what one forward batch gives the backbone
    counts = {}

    def forward_pass():
        n = 0
        for i0, i1, pl in fwd:
            n += len(bench.planted_step(model, i0, i1, pl, True)['mkpts0_f'])
        counts['forward'] = n

    def feature_pass():
        recs = []
        for s in range(0, K, chunk):
            for k, r in enumerate(model.extract_features(images[s:s + chunk]), s):
                recs.append(ImageFeatures(torch.add(pc[k], r.coarse, alpha=0.0), torch.add(pf[k], r.fine, alpha=0.0), r.image_size))
        n = 0
        for bt in batches:
            n += len(model.match_features([recs[p[0]] for p in bt], [recs[p[1]] for p in bt])['mkpts0_f'])
        counts['features'] = n
    with torch.no_grad():
        rates = alternate({'forward': rate_window(forward_pass, len(pairs), passes), 'features': rate_window(feature_pass, len(pairs), passes)},
                          warmup=1)
    log(f'({tag}) {len(pairs)} pairs over {K} images of 640 x 640, fp16, batches of {batch}, thresholds 0.2 / 0.1, planted maps; '
        f'{WINDOWS} windows of {passes} passes per form, alternating; fine matches per pass: forward {counts["forward"]}, features {counts["features"]}')
    log(stat('backbone per pair batch + forward_features (planted_step)', rates['forward'], 'pairs/s'))
    log(stat(f'extract_features once per image ({K} extractions per pass) + match_features', rates['features'], 'pairs/s'))
    return verdict(log, 'kept features against forward (pairs/s; ratio = features / forward)', rates['forward'], rates['features'], True)


def model_legs(log, legs):
    import bench
    model = bench.build_model('fp16', 0.2, 0.1, DEV)[0]
    if 'allpairs' in legs:
        K = 16
        i0, i1 = bench.synth_pairs(K // 2, 5, 640, DEV)
        pc, pf = planted_images(K)
        pairs_leg(log, '1', model, torch.cat([i0, i1]), pc, pf, [(i, j) for i in range(K) for j in range(i + 1, K)], 8, 2)
        del pc, pf
        torch.cuda.empty_cache()
    if 'query' in legs:
        K = 51
        i0, i1 = bench.synth_pairs(26, 6, 640, DEV)
        pc, pf = planted_images(K, seed=60001)
        pairs_leg(log, '3', model, torch.cat([i0, i1])[:K], pc, pf, [(0, k) for k in range(1, K)], 10, 4)


def invariance_leg(log):
    import bench
    log('(4) is extract_features(image) at batch 1 bit-equal to the same image inside a batch of 4?  (the fused inference backbone)')
    for mode in ('fp16', 'bf16'):
        model = bench.build_model(mode, 0.0, 0.0, DEV)[0]
        for h, w in ((160, 184), (640, 640)):
            g = torch.Generator().manual_seed(h + w)
            imgs = torch.rand(4, 1, h, w, generator=g).to(DEV)
            with torch.no_grad():
                inside = model.extract_features(imgs)
                alone = [model.extract_features(imgs[k:k + 1])[0] for k in range(4)]
            res = []
            for name in ('coarse', 'fine'):
                same = all(torch.equal(getattr(a, name), getattr(b, name)) for a, b in zip(alone, inside))
                worst = max(float((getattr(a, name).float() - getattr(b, name).float()).abs().max()) for a, b in zip(alone, inside))
                res.append(f'{name} map {"equal" if same else f"DIFFERENT (largest difference {worst:.3g})"}')
            log(f'  {mode} {h} x {w}: ' + ', '.join(res))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--legs', default='kernels,allpairs,query,invariance', help='comma-separated subset of kernels, allpairs, query, invariance')
    args = ap.parse_args(argv)
    legs = set(args.legs.split(','))
    if legs - {'kernels', 'allpairs', 'query', 'invariance'}:
        raise SystemExit(f'unknown legs: {sorted(legs - {"kernels", "allpairs", "query", "invariance"})}')
    if not torch.cuda.is_available():
        raise SystemExit('feature_cache_probe: needs an MI355X (no CPU path, no CPU numbers)')
    from geoformer_amd import miopen
    miopen.use_shipped_find_db()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                       # rewritten line by line: a leg that fails leaves the legs before it on record
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    log(f'feature_cache_probe on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; legs: {", ".join(sorted(legs))}')
    if 'kernels' in legs:
        kernel_leg(log)
    if legs & {'allpairs', 'query'}:
        model_legs(log, legs)
    if 'invariance' in legs:
        invariance_leg(log)
    missing = {'kernels', 'allpairs', 'query', 'invariance'} - legs
    if missing:
        log(f'not measured in this run: {", ".join(sorted(missing))}')


if __name__ == '__main__':
    main()
