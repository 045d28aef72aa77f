"""What BatchNorm recalibration moves and what it costs: python tools/bn_recal_ab.py [--steps K] [--batch B] [--n N] [--rounds R] [--out FILE]
CIFAR-15, fp32, one model trained for K captured steps (default 300) with --ema-decay 0.99 on N synthetic batches of B images, visited in
turn. Then, on a fixed synthetic test set of 4 x 256 images and one noise seed:
  1. the test-pass ELBO of the averaged weights with the live weights' BatchNorm statistics, and recalibrated on the first N training
     batches (evaluate.test_pass(bn_recal=...), what --ema-bn-batches N does), and the live weights' own ELBO beside them;
  2. the time of one N-round recalibration (recalibrate.recalibrate_bn on the averaged weights: train-mode forwards, N folds, one finish; as
     the call picks it, replayed from round 3 on when N >= 8, and launched eagerly) beside N eval-mode forwards of the same batches: R rounds,
     the three alternated inside each round, each between two device events; medians and the spread.
Writes everything to FILE (profiles/bn_recal.txt). Measurement tooling only; bench.py has no such flag and stays the yardstick."""
import argparse
import os
import statistics
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import torch  # noqa: E402

import lvae_amd  # noqa: E402,F401
from lvae_amd.configs import CIFAR15, synthetic_images  # noqa: E402
from lvae_amd.engine import TrainStep  # noqa: E402
from lvae_amd.evaluate import test_pass  # noqa: E402
from lvae_amd.models.lvae import LadderVAE  # noqa: E402
from lvae_amd.noise import PhiloxNoise  # noqa: E402
from lvae_amd.optim import Adamax  # noqa: E402
from lvae_amd.passes import eval_mode  # noqa: E402
from lvae_amd.recalibrate import recalibrate_bn, restore_bn  # noqa: E402


def between_events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--n', type=int, default=20, help='batches of a recalibration')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(root, 'profiles', 'bn_recal.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('this measurement needs the GPU: nothing is timed without one')
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(1234)
    train = [synthetic_images(CIFAR15, args.batch, gen).to(dev) for _ in range(args.n)]
    tests = [synthetic_images(CIFAR15, 256, torch.Generator().manual_seed(99 + i)).to(dev) for i in range(4)]
    torch.manual_seed(42)
    model = LadderVAE(**CIFAR15).to(dev)
    model.train()
    model.noise = PhiloxNoise(seed=42, rank=0)
    opt = Adamax(model, lr=3e-4, ema_decay=0.99)
    step = TrainStep(model, opt, use_graph=True)
    for i in range(args.steps):
        out = step(train[i % args.n])
    torch.cuda.synchronize()
    lines = ['CIFAR-15 fp32, %d captured steps of batch %d on %d synthetic batches, Adamax lr 3e-4, --ema-decay 0.99, on %s.'
             % (args.steps, args.batch, args.n, torch.cuda.get_device_name(0)),
             'last training step: loss %.4f   ELBO %.4f' % (float(out['loss']), float(out['elbo'])), '',
             'Test pass, 1 sample, %d synthetic test images, one noise seed:' % sum(t.shape[0] for t in tests)]
    live = test_pass(model, tests, 1, noise=PhiloxNoise(seed=21))
    plain = test_pass(model, tests, 1, noise=PhiloxNoise(seed=21), optimizer=opt)
    recal = test_pass(model, tests, 1, noise=PhiloxNoise(seed=21), optimizer=opt, bn_recal=lambda: train)
    for tag, r in (('live weights, live statistics', live), ('averaged weights, live statistics', plain),
                   ('averaged weights, recalibrated on %d batches' % recal['bn_recal/rounds'], recal)):
        lines.append('  %-48s ELBO %.4f   recons %.4f   KL %.4f' % (tag, r['elbo/elbo'], r['elbo/recons'], r['elbo/kl']))
    lines += ['  recalibrated - live statistics, averaged weights: %+.4f nats per image' % (recal['elbo/elbo'] - plain['elbo/elbo']), '']

    def forwards():
        with torch.no_grad(), eval_mode(model):
            for x in train:
                model(x)

    rows = []
    with opt.swap_ema():
        forwards()                                     # warm-up of the eval-mode shapes; the recalibrations warmed theirs above
        recalibrate_bn(model, train, use_graph=False)
        restore_bn(model)
        for _ in range(args.rounds):
            a = between_events(lambda: recalibrate_bn(model, train))
            restore_bn(model)
            b = between_events(lambda: recalibrate_bn(model, train, use_graph=False))
            restore_bn(model)
            c = between_events(forwards)
            rows.append((a, b, c))
    lines += ['One recalibration on %d batches of %d (averaged weights) beside %d eval-mode forwards of the same batches,' % (args.n, args.batch, args.n),
              '%d rounds, the three alternated inside a round, each between two device events, ms:' % args.rounds, '']
    lines += ['  round %d   recalibration %.2f   recalibration, eager %.2f   eval forwards %.2f' % (i + 1, a, b, c) for i, (a, b, c) in enumerate(rows)]
    med = [statistics.median(r[j] for r in rows) for j in range(3)]
    spread = [max(r[j] for r in rows) - min(r[j] for r in rows) for j in range(3)]
    lines += ['', '  median    recalibration %.2f   recalibration, eager %.2f   eval forwards %.2f' % tuple(med),
              '  max - min recalibration %.2f   recalibration, eager %.2f   eval forwards %.2f' % tuple(spread),
              '  (the recalibration as the call picks it runs two rounds eagerly, captures one and replays it %d times; the capture is in its time)'
              % max(0, args.n - 3)]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
