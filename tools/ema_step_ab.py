"""Step time with the weight average on: python tools/ema_step_ab.py <ema_decay> [bench.py arguments]
Runs bench.py's main() with every Adamax it builds constructed with ema_decay=<ema_decay> (0 = the product default, the plain kernel).
bench.py itself has no such flag and stays the yardstick. Measurement tooling only (profiles/ema_step_ab.txt)."""
import functools
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
decay = float(sys.argv[1])
sys.argv = ['bench.py'] + sys.argv[2:]
import bench  # noqa: E402  (imports the package)
from lvae_amd import optim  # noqa: E402

_init = optim.Adamax.__init__


@functools.wraps(_init)
def _with_average(self, model, *a, **kw):
    kw.setdefault('ema_decay', decay)
    _init(self, model, *a, **kw)


optim.Adamax.__init__ = _with_average
bench.main()
