"""Test-pass time with image quality on: python tools/image_quality_ab.py [--pairs P] [--batches K] [--batch B] [--samples S] [--out FILE]
Interleaved pairs of evaluate.test_pass on bench.py's CIFAR-15 model (fp32, one GPU, captured sample graphs) without and with a
quality.ImageQuality, in ONE process on ONE model: both forms are warmed up (their graphs captured), then P times: one timed pass of K
batches of B images without the object, one with it. A pass is timed between two device events on the stream it is issued from; it ends in
its device-to-host copy, so the events enclose all of its work. Prints each pair, the medians, the median difference and ratio, and the
spread of the plain pass in those same pairs, and the time of the quality launches alone on a batch. Measurement tooling only
(profiles/image_quality_ab.txt)."""
import argparse
import os
import statistics
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402

import bench  # noqa: E402  (imports the package)
from lvae_amd.evaluate import test_pass  # noqa: E402
from lvae_amd.models.lvae import LadderVAE  # noqa: E402
from lvae_amd.noise import PhiloxNoise  # noqa: E402
from lvae_amd.quality import ImageQuality  # noqa: E402


def timed(fn, dev):
    """(ms between two device events around fn(), what fn returned)"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    res = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=6)
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--batch', type=int, default=1000)
    ap.add_argument('--samples', type=int, default=1)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.manual_seed(42)
    model = LadderVAE(**bench.CIFAR15).to(dev)
    model.train()
    model.noise = PhiloxNoise(seed=42)
    model.pack()
    quality = ImageQuality(dev)
    noise = PhiloxNoise(seed=7)
    xs = [b.to(dev) for b in bench.synth_batches(args.batches, args.batch, 1234)]
    forms = {'plain': None, 'quality': quality}

    def one(tag):
        return timed(lambda: test_pass(model, xs, args.samples, noise=noise, image_quality=forms[tag]), dev)

    for tag in forms:                                # captures the plan of each form, then one replayed pass
        one(tag)
        one(tag)
    lines = ['# ms per test pass of %d batches x %d images, %d sample(s) per image, interleaved in one process, device events' % (
        args.batches, args.batch, args.samples), '# pair   plain   quality   difference']
    ms = {'plain': [], 'quality': []}
    res = None
    for p in range(args.pairs):
        for tag in forms:
            dt, r = one(tag)
            ms[tag].append(dt)
            res = r if tag == 'quality' else res
        lines.append('%4d   %9.3f   %9.3f   %+9.3f' % (p, ms['plain'][-1], ms['quality'][-1], ms['quality'][-1] - ms['plain'][-1]))
    diffs = [b - a for a, b in zip(ms['plain'], ms['quality'])]
    mp, mq = statistics.median(ms['plain']), statistics.median(ms['quality'])
    lines.append('median plain %.3f ms   median quality %.3f ms   median difference %+.3f ms   ratio of medians %.4f' % (
        mp, mq, statistics.median(diffs), mq / mp))
    lines.append('spread of the plain pass over the pairs: min %.3f   max %.3f   (max - min %.3f ms)' % (
        min(ms['plain']), max(ms['plain']), max(ms['plain']) - min(ms['plain'])))
    # the launches alone: one batch against a shifted copy of itself, channel-last as the pass holds them
    a = xs[0].permute(0, 2, 3, 1).contiguous()
    b = a.roll(1, 0)
    alone = []
    for _ in range(2 + args.pairs):
        alone.append(timed(lambda: quality.fold(a, b, channel_last=True), dev)[0])
    quality.reset()
    N, H, W, C = a.shape
    lines.append('quality + fold launches alone on one batch of %d x %d x %d x %d: median %.3f ms (min %.3f); they read %.1f MB and take '
                 '%.2f Gflop (121 taps of both images, twice: 16 flop per tap, at %d positions)' % (
                     N, C, H, W, statistics.median(alone[2:]), min(alone[2:]), 2 * a.numel() * 4 / 1e6,
                     N * C * (H - 10) * (W - 10) * 121 * 16 / 1e9, N * C * (H - 10) * (W - 10)))
    lines.append('the last pass (untrained weights): PSNR %.2f dB   SSIM %.4f over %d images' % (
        res['quality/psnr'], res['quality/ssim'], res['n_images']))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
