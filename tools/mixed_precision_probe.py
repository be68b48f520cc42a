"""What the bf16-backbone / fp16-matching mode ('bf16_fp16') costs against the two single-type 16-bit modes, measured in ONE process
so that the forms compared share the machine's state:   python tools/mixed_precision_probe.py [--repeats 7] [--out FILE]

  (a) gf_fine_gather at the nominal load (8 pairs x 2300 matches, C = 128, CC = 256, channels-last 320 x 320 fine maps): the row
      kernel fp16 -> fp16 and bf16 -> bf16 (copies), bf16 -> fp16 (converting in registers), and bf16 -> fp16 through the general
      kernel (the same maps as a non-channels-last copy);
  (b) gf_pos_encode on [16, 256, 80, 80] channels-last maps, same-type and converting;
  (c) pairs/s of the three 16-bit modes at 480 x 640 / 480 x 608 batch 1 and at 640 x 640 batch 8: `forward` = GeoFormer.forward on
      synthetic image pairs with thresholds 0 / 0; `nominal` = backbone on the images + matching path on planted-correspondence maps
      (thresholds 0.2 / 0.1, thousands of matches per pair: bench.py's construction), the maps in the mode's backbone dtype.

Method: every form is warmed up, then timed in `repeats` rounds; within a round the forms run one after the other, so a drift of the
machine hits all of them.  Kernel times are HIP events around back-to-back launches, as many as fill about 0.15 s per form and round
(ops.fine_gather takes its two outputs from torch's caching allocator on every call, as the model's call does: the same blocks come
back without any device work, and the host's part of a call stays below the kernel's time, so the queue never runs dry); pairs/s is
a host clock around steps that end in the forward's own host synchronisation.  Reported: median, minimum and maximum over the rounds - the spread is the
yardstick for any difference between two forms.  Bytes are counted from the shapes (what the kernel must move), not measured."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

DEV = 'cuda:0'
F16, BF16 = torch.float16, torch.bfloat16
NAME = {F16: 'fp16', BF16: 'bf16'}


def time_kernels(forms, repeats, window_s=0.15, warmup=5):
    """forms: {name: fn}.  -> ({name: [us per call, one value per round]}, {name: calls per round}).  A form's timed window is sized
    from a first timing of its own to about `window_s` seconds of back-to-back launches: a window of a few milliseconds measures the
    clock's ramp and the scheduler as much as the kernel."""
    def timed(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / calls
    calls = {}
    for name, fn in forms.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(20, int(window_s * 1e6 / timed(fn, 20)))
    out = {k: [] for k in forms}
    for _ in range(repeats):
        for name, fn in forms.items():
            out[name].append(timed(fn, calls[name]))
    return out, calls


def line(name, us, nbytes=None):
    med = statistics.median(us)
    s = f'  {name:<44s} {med:8.1f} us  (min {min(us):.1f}, max {max(us):.1f}, spread {100 * (max(us) - min(us)) / med:.1f} %)'
    if nbytes:
        s += f'   {nbytes / med / 1e3:6.0f} GB/s over {nbytes / 1e6:.0f} MB'
    return s


def fine_gather_leg(log, repeats):
    from geoformer_amd import ops
    N, C, CC, hc, M = 8, 128, 256, 80, 8 * 2300
    g = torch.Generator().manual_seed(1)
    f32 = [torch.randn(N, C, 4 * hc, 4 * hc, generator=g) for _ in range(2)]
    c32 = [torch.randn(N, hc * hc, CC, generator=g) for _ in range(2)]
    b = torch.arange(N).repeat_interleave(M // N).to(DEV)
    i, j = (torch.randint(0, hc * hc, (M,), generator=g).to(DEV) for _ in range(2))
    maps = {dt: [t.to(DEV, dt).contiguous(memory_format=torch.channels_last) for t in f32] for dt in (F16, BF16)}
    nchw = [t.contiguous() for t in maps[BF16]]
    ctx = {dt: [t.to(DEV, dt) for t in c32] for dt in (F16, BF16)}

    def form(fm, out):
        return lambda: ops.fine_gather(fm[0], fm[1], ctx[out][0], ctx[out][1], b, i, j, hc, hc, 4, 5, out)
    forms = {'rows fp16 -> fp16 (copy)': form(maps[F16], F16), 'rows bf16 -> bf16 (copy)': form(maps[BF16], BF16),
             'rows bf16 -> fp16 (converting)': form(maps[BF16], F16), 'general kernel bf16 -> fp16 (NCHW maps)': form(nchw, F16)}
    assert torch.equal(forms['rows bf16 -> fp16 (converting)']()[0], forms['general kernel bf16 -> fp16 (NCHW maps)']()[0])
    # per window: 25 x C elements read (2 B) and written (2 B); per match and side one coarse row read and written
    nbytes = 2 * M * (25 * C * (2 + 2) + CC * (2 + 2))
    us, calls = time_kernels(forms, repeats)
    log(f'(a) gf_fine_gather, {N} pairs x {M // N} matches = {2 * M} windows of 25 x {C}, coarse rows of {CC}; {repeats} rounds of '
        f'{min(calls.values())}-{max(calls.values())} calls (about 0.15 s) per form')
    for k, v in us.items():
        log(line(k, v, nbytes))
    same, conv, gen = (statistics.median(us[k]) for k in ('rows bf16 -> bf16 (copy)', 'rows bf16 -> fp16 (converting)',
                                                          'general kernel bf16 -> fp16 (NCHW maps)'))
    spread = max(max(v) - min(v) for k, v in us.items() if k.startswith('rows'))
    log(f'  converting rows - bf16 copy rows = {conv - same:+.1f} us (difference of the medians) against a round-to-round spread of {spread:.1f} us '
        f'(the largest max - min over the rounds among the three row forms): {"inside" if abs(conv - same) <= spread else "OUTSIDE"} the spread; '
        f'general kernel / converting rows = {gen / conv:.2f} x (medians)')


def pos_encode_leg(log, repeats):
    from geoformer_amd import ops
    N, C, H, W = 16, 256, 80, 80
    g = torch.Generator().manual_seed(2)
    x32 = torch.randn(N, C, H, W, generator=g)
    pe = torch.randn(H, W, C, generator=g).to(DEV)
    x = {dt: x32.to(DEV, dt).contiguous(memory_format=torch.channels_last) for dt in (F16, BF16)}
    outs = {dt: torch.empty(N, H * W, C, dtype=dt, device=DEV) for dt in (F16, BF16)}
    forms = {f'{NAME[a]} -> {NAME[o]}': (lambda a=a, o=o: ops.pos_encode(x[a], pe, o, outs[o]))
             for a, o in ((F16, F16), (BF16, BF16), (BF16, F16), (F16, BF16))}
    nbytes = N * H * W * C * (2 + 2) + H * W * C * 4          # maps in and out; the fp32 table once (it stays in cache across the batch)
    us, calls = time_kernels(forms, repeats)
    log(f'(b) gf_pos_encode, [{N}, {C}, {H}, {W}] channels-last -> [{N}, {H * W}, {C}]; {repeats} rounds of '
        f'{min(calls.values())}-{max(calls.values())} calls (about 0.15 s) per form')
    for k, v in us.items():
        log(line(k, v, nbytes))


def forward_leg(log, repeats, steps):
    import bench
    modes = ('fp16', 'bf16', 'bf16_fp16')
    for tag, batch, hw0, hw1 in (('480 x 640 / 480 x 608, batch 1', 1, (480, 640), (480, 608)), ('640 x 640, batch 8', 8, (640, 640), (640, 640))):
        if hw0 == hw1:
            i0, i1 = bench.synth_pairs(batch, 5, hw0[0], DEV)
        else:
            i0, i1 = bench.synth_rect_pair(hw0, hw1, 77, DEV)
        (h0, w0), (h1, w1) = (hw0[0] // 8, hw0[1] // 8), (hw1[0] // 8, hw1[1] // 8)
        g = torch.Generator().manual_seed(70000)
        big = torch.randn(batch, 256, h0 + 1, w0 + 1, generator=g) * 0.5
        bigf = torch.randn(batch, 128, 4 * (h0 + 1), 4 * (w0 + 1), generator=g)
        planted32 = (big[:, :, :h0, :w0], bigf[:, :, :4 * h0, :4 * w0],
                     big[:, :, 1:1 + h1, 1:1 + w1] + 0.35 * torch.randn(batch, 256, h1, w1, generator=g),
                     bigf[:, :, 4:4 + 4 * h1, 4:4 + 4 * w1] + 0.35 * torch.randn(batch, 128, 4 * h1, 4 * w1, generator=g))
        steps_of, matches = {}, {}
        for mode in modes:
            light, nominal = bench.build_model(mode, 0.0, 0.0, DEV)[0], bench.build_model(mode, 0.2, 0.1, DEV)[0]
            pl = [t.to(DEV, nominal.backbone_dtype).contiguous(memory_format=torch.channels_last) for t in planted32]

            def nominal_step(m=nominal, pl=pl):
                if hw0 == hw1:
                    fc, ff = m._backbone(torch.cat([i0, i1], 0))
                    (fc0, fc1), (ff0, ff1) = fc.split(batch), ff.split(batch)
                else:
                    (fc0, ff0), (fc1, ff1) = m._backbone_unequal(i0, i1)
                return m.forward_features({'image0': i0, 'image1': i1}, torch.add(pl[0], fc0, alpha=0.0), torch.add(pl[1], ff0, alpha=0.0),
                                          torch.add(pl[2], fc1, alpha=0.0), torch.add(pl[3], ff1, alpha=0.0))
            steps_of[('forward', mode)] = lambda m=light: m({'image0': i0, 'image1': i1})
            steps_of[('nominal', mode)] = nominal_step
        rates = {k: [] for k in steps_of}
        with torch.no_grad():
            for k, fn in steps_of.items():
                for _ in range(3):
                    out = fn()
                matches[k] = len(out['b_ids']) / batch
            torch.cuda.synchronize()
            for _ in range(repeats):
                for k, fn in steps_of.items():
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(steps):
                        fn()                              # ends in the forward's own host synchronisation (the number of fine matches)
                    torch.cuda.synchronize()
                    rates[k].append(batch * steps / (time.perf_counter() - t))
        log(f'(c) {tag}: pairs/s on one stream, {repeats} rounds of {steps} steps')
        for k, v in rates.items():
            med = statistics.median(v)
            log(f'  {k[0]:<8s} {k[1]:<10s} {med:8.1f} pairs/s  (min {min(v):.1f}, max {max(v):.1f}, spread {100 * (max(v) - min(v)) / med:.1f} %)   '
                f'{matches[k]:.0f} coarse matches per pair')
        del steps_of
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--skip-forward', action='store_true', help='kernels only: legs (a) and (b)')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('mixed_precision_probe: needs an MI355X (no CPU path, no CPU numbers)')
    from geoformer_amd import miopen
    miopen.use_shipped_find_db()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    log(f'mixed_precision_probe on {torch.cuda.get_device_name(0)}, torch {torch.__version__}')
    fine_gather_leg(log, args.repeats)
    pos_encode_leg(log, args.repeats)
    if not args.skip_forward:
        forward_leg(log, args.repeats, args.steps)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
