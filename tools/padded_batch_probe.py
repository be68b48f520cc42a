"""What batching pairs of UNEQUAL image sizes on a padded canvas buys and costs, measured in ONE process so that the forms compared share
the machine's state:   python tools/padded_batch_probe.py [--out profiles/padded_batch.txt] [--legs kernels,pairs,kept]

  (a) the two ragged kernels against their address-table siblings on EQUAL-shape maps (what the per-sample record costs when nothing is
      padded), at the nominal loads of profiles/feature_cache.txt: gf_pos_encode_* on 16 maps of [256, 80, 80], gf_fine_gather_* on
      36800 windows of 25 x 128.
  (b) all 120 pairs of 16 images of 8 distinct sizes (height 480, widths 512 .. 736 in steps of 32, two images each; fp16, thresholds
      0.2 / 0.1 as bench.py's default load, planted correspondences): pairs/s and fine matches per pair of
      GeoFormer.match_features(pad=True) on matcher.group_pairs_padded's batches for max_waste in {1.1, 1.25, 1.5, 2}, against pad=False on
      matcher.group_pairs' batches (pairs of one shape pair only) - same records, same run.  Each pass extracts the 16 images first
      (one backbone call per size), inside the timed window, as a caller with a feature store pays it.
  (c) the share of a pair's coarse matches that it keeps when it runs in a padded batch instead of alone (batch 1, no padding): matches
      compared as (cell of image 0, cell of image 1) in the pair's own coordinates.  Not a gate: masked attention sums in another order,
      and the device RANSAC draws its samples per position in the batch (as in any batched forward).

Method as tools/feature_cache_probe.py: every form is warmed up; then 7 windows per form, the forms alternating window by window;
kernel windows are 100 back-to-back launches between two device events, pairs/s windows a host clock around whole passes closed by a
device synchronise.  Reported: median with minimum .. maximum over the windows.

Planted maps: image k's maps are crops (60 x w_k / 8 cells) of one random map shifted by k % 9 coarse cells plus noise, so that any two
images correspond by a translation where they overlap; every map the matching path reads is `planted + 0 * backbone output` in an
allocation of its own."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from feature_cache_probe import DEV, F16, WINDOWS, alternate, kernel_window, rate_window, stat, verdict  # noqa: E402

WASTES = (1.1, 1.25, 1.5, 2.0)
HEIGHT, WIDTHS = 480, tuple(range(512, 737, 32))


def kernel_leg(log):
    from geoformer_amd import ops
    g = torch.Generator().manual_seed(2)
    N, C, H, W = 16, 256, 80, 80
    maps = [(torch.randn(H, W, C, generator=g)).to(DEV, F16).permute(2, 0, 1) for _ in range(N)]          # 16 allocations
    pe = torch.randn(H, W, C, generator=g).to(DEV)
    out = torch.empty(N, H * W, C, dtype=F16, device=DEV)
    mask = torch.empty(N, H, W, dtype=torch.bool, device=DEV)
    table, ragged = ops.MapBatch(maps), ops.RaggedMapBatch(maps)
    table.table(), ragged.table()
    assert torch.equal(ops.pos_encode(ragged, pe, F16, mask_out=mask), ops.pos_encode(table, pe, F16)) and bool(mask.all())
    us = alternate({'table': kernel_window(lambda: ops.pos_encode(table, pe, F16, out)),
                    'ragged': kernel_window(lambda: ops.pos_encode(ragged, pe, F16, out)),
                    'ragged_mask': kernel_window(lambda: ops.pos_encode(ragged, pe, F16, out, mask))})
    log(f'(a1) position encoding, {N} separate maps of [{C}, {H}, {W}] channels-last fp16 -> fp16 (equal shapes: nothing is padded); '
        f'{WINDOWS} windows of 100 launches per form, alternating')
    log(stat('gf_pos_encode_ptrs', us['table'], 'us'))
    log(stat('gf_pos_encode_ragged', us['ragged'], 'us'))
    log(stat('gf_pos_encode_ragged writing the mask too', us['ragged_mask'], 'us'))
    verdict(log, 'ragged entry against table entry (us; ratio = table / ragged)', us['table'], us['ragged'], False)

    Nf, Cf, CC, hc, M = 8, 128, 256, 80, 8 * 2300
    f0 = [torch.randn(4 * hc, 4 * hc, Cf, generator=g).to(DEV, F16).permute(2, 0, 1) for _ in range(Nf)]
    f1 = [torch.randn(4 * hc, 4 * hc, Cf, generator=g).to(DEV, F16).permute(2, 0, 1) for _ in range(Nf)]
    c0, c1 = (torch.randn(Nf, hc * hc, CC, generator=g).to(DEV, F16) for _ in range(2))
    b = torch.arange(Nf).repeat_interleave(M // Nf).to(DEV)
    i, j = (torch.randint(0, hc * hc, (M,), generator=g).to(DEV) for _ in range(2))
    t0, t1, r0, r1 = ops.MapBatch(f0), ops.MapBatch(f1), ops.RaggedMapBatch(f0), ops.RaggedMapBatch(f1)
    for t in (t0, t1, r0, r1):
        t.table()
    args = (c0, c1, b, i, j, hc, hc, 4, 5, F16)
    assert all(torch.equal(x, y) for x, y in zip(ops.fine_gather(r0, r1, *args), ops.fine_gather(t0, t1, *args)))
    us = alternate({'table': kernel_window(lambda: ops.fine_gather(t0, t1, *args)),
                    'ragged': kernel_window(lambda: ops.fine_gather(r0, r1, *args))})
    log(f'(a2) fine gather, {Nf} pairs x {M // Nf} matches = {2 * M} windows of 25 x {Cf}, coarse rows of {CC}, fp16 -> fp16 (one wave per window), '
        f'2 x {Nf} separate maps of equal shape; {WINDOWS} windows of 100 launches per form, alternating')
    log(stat('gf_fine_gather_ptrs', us['table'], 'us'))
    log(stat('gf_fine_gather_ragged', us['ragged'], 'us'))
    verdict(log, 'ragged entry against table entry (us; ratio = table / ragged)', us['table'], us['ragged'], False)


def planted_maps(sizes, seed=61000, noise=0.25):
    """sizes: [(h, w)] of the images -> per image (coarse [256, h/8, w/8], fine [128, h/2, w/2]) fp16 channels-last on the device."""
    g = torch.Generator().manual_seed(seed)
    gh, gw = max(h for h, _ in sizes) // 8 + 8, max(w for _, w in sizes) // 8 + 8
    big = torch.randn(256, gh, gw, generator=g) * 0.5
    bigf = torch.randn(128, 4 * gh, 4 * gw, generator=g)
    out = []
    for k, (h, w) in enumerate(sizes):
        s, hc, wc = k % 9, h // 8, w // 8
        c = (big[:, s:s + hc, s:s + wc] + noise * torch.randn(256, hc, wc, generator=g)).to(F16)
        f = (bigf[:, 4 * s:4 * (s + hc), 4 * s:4 * (s + wc)] + noise * torch.randn(128, 4 * hc, 4 * wc, generator=g)).to(F16)
        out.append((c.permute(1, 2, 0).contiguous().to(DEV).permute(2, 0, 1), f.permute(1, 2, 0).contiguous().to(DEV).permute(2, 0, 1)))
    return out


def model_legs(log, legs):
    import bench
    from geoformer_amd.matcher import DEFAULT_PAD_WASTE, group_pairs, group_pairs_padded
    from geoformer_amd.model.full_model import ImageFeatures
    model = bench.build_model('fp16', 0.2, 0.1, DEV)[0]
    sizes = [(HEIGHT, w) for w in WIDTHS for _ in range(2)]
    K = len(sizes)
    g = torch.Generator().manual_seed(9)
    images = [torch.rand(1, 1, h, w, generator=g).to(DEV) for h, w in sizes]
    planted = planted_maps(sizes)
    pairs = [(i, j) for i in range(K) for j in range(i + 1, K)]
    shapes = [(sizes[i], sizes[j]) for i, j in pairs]
    groupings = {'exact': group_pairs(shapes, 8)}
    for r in WASTES:
        groupings[f'pad_{r}'] = group_pairs_padded(shapes, 8, r)

    def extract():
        recs = [None] * K
        for s in range(0, K, 2):                         # the two images of one size in one backbone call
            for k, r in enumerate(model.extract_features(torch.cat(images[s:s + 2])), s):
                recs[k] = ImageFeatures(torch.add(planted[k][0], r.coarse, alpha=0.0), torch.add(planted[k][1], r.fine, alpha=0.0), r.image_size)
        return recs

    def run(recs, batches, pad):
        outs = []
        for idx in batches:
            outs.append(model.match_features([recs[pairs[k][0]] for k in idx], [recs[pairs[k][1]] for k in idx], pad=pad))
        return outs

    counts = {}

    def make_pass(name):
        def one_pass():
            counts[name] = sum(len(d['mkpts0_f']) for d in run(extract(), groupings[name], name != 'exact'))
        return one_pass
    with torch.no_grad():
        if 'pairs' in legs:
            passes = 2
            rates = alternate({name: rate_window(make_pass(name), len(pairs), passes) for name in groupings}, warmup=1)
            log(f'(b) {len(pairs)} pairs over {K} images of {len(WIDTHS)} sizes ({HEIGHT} x {WIDTHS[0]} .. {WIDTHS[-1]}, two each), fp16, batches of at most 8, '
                f'thresholds 0.2 / 0.1, planted maps; every pass extracts the {K} images first; {WINDOWS} windows of {passes} passes per form, alternating')
            for name, batches in groupings.items():
                what = ('pad=False, group_pairs (one shape pair per batch)' if name == 'exact'
                        else f'pad=True, group_pairs_padded(max_waste={name[4:]})')
                log(stat(f'{what}: {len(batches)} model calls', rates[name], 'pairs/s') + f'; fine matches per pair {counts[name] / len(pairs):.1f}')
            best = max((n for n in groupings if n != 'exact'), key=lambda n: statistics.median(rates[n]))
            verdict(log, f'best padded candidate ({best}) against pad=False (pairs/s; ratio = padded / exact)', rates['exact'], rates[best], True)
            log(f'  matcher.DEFAULT_PAD_WASTE in this tree: {DEFAULT_PAD_WASTE}')
        if 'kept' in legs:
            recs = extract()
            alone = run(recs, [[k] for k in range(len(pairs))], False)
            log(f'(c) share of a pair\'s coarse matches (cell of image 0, cell of image 1) that it keeps in a padded batch, against the pair run alone '
                f'at batch 1; {len(pairs)} pairs, mean of {statistics.mean(len(d["b_ids"]) for d in alone):.1f} coarse matches per pair alone')
            for r in WASTES:
                batches = groupings[f'pad_{r}']
                shares, sizes_in = [], []
                for idx, d in zip(batches, run(recs, batches, True)):
                    w0, w1 = int(d['hw0_c'][1]), int(d['hw1_c'][1])
                    bb, ii, jj = d['b_ids'].tolist(), d['i_ids'].tolist(), d['j_ids'].tolist()
                    for n, k in enumerate(idx):
                        got = {(i // w0, i % w0, j // w1, j % w1) for b_, i, j in zip(bb, ii, jj) if b_ == n}
                        a = alone[k]
                        a0, a1 = int(a['hw0_c'][1]), int(a['hw1_c'][1])
                        want = {(i // a0, i % a0, j // a1, j % a1) for i, j in zip(a['i_ids'].tolist(), a['j_ids'].tolist())}
                        if want:
                            shares.append(len(want & got) / len(want))
                        sizes_in.append(len(got))
                log(f'  max_waste {r:<5}: {len(batches)} batches; kept share mean {100 * statistics.mean(shares):.2f} %, median {100 * statistics.median(shares):.2f} %, '
                    f'minimum {100 * min(shares):.2f} %; coarse matches per pair in the batch {statistics.mean(sizes_in):.1f}')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--legs', default='kernels,pairs,kept', help='comma-separated subset of kernels, pairs, kept')
    args = ap.parse_args(argv)
    legs = set(args.legs.split(','))
    if legs - {'kernels', 'pairs', 'kept'}:
        raise SystemExit(f'unknown legs: {sorted(legs - {"kernels", "pairs", "kept"})}')
    if not torch.cuda.is_available():
        raise SystemExit('padded_batch_probe: needs an MI355X (no CPU path, no CPU numbers)')
    from geoformer_amd import miopen
    miopen.use_shipped_find_db()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                       # rewritten line by line: a leg that fails leaves the legs before it on record
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    log(f'padded_batch_probe on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; legs: {", ".join(sorted(legs))}')
    if 'kernels' in legs:
        kernel_leg(log)
    if legs & {'pairs', 'kept'}:
        model_legs(log, legs)
    missing = {'kernels', 'pairs', 'kept'} - legs
    if missing:
        log(f'not measured in this run: {", ".join(sorted(missing))}')


if __name__ == '__main__':
    main()
