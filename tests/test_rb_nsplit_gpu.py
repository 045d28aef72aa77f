"""Two workgroups per tile in the whole-image plain launches (csrc/resblock_img.hip, rb_conv_kernel NS == 2; lvae_rb_ext.nsplit): each computes one
32-channel half of the tile's output. lvae_resblock_conv_f32 is driven directly with nsplit = 1 and nsplit = 2 on identical inputs: everything
either form writes must be bit for bit the same (the k-split, the order of the four partial tiles and the per-channel order of the statistics
are unchanged), everything written once per tile or once per launch must be written once, and y must sit inside the bound the kernel's own
tests hold it to against float64 (tests/test_resblock_img_gpu.py: 2e-6 for conv1's forward launch, 3 x 4e-6 for the gate-backward launch's dh2,
3 x 8e-6 for the BatchNorm-apply launch's dh1; norm-relative)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CH = 64
GUARD = 64   # NaN rows behind every output: a partial 32-pixel tile has up to 31 rows past the batch
SHAPES = [(1, 2, 2), (8, 2, 2), (9, 2, 2), (2, 4, 4), (3, 4, 4), (3, 8, 8)]
PROLOGUES = ['none', 'coef', 'fold1', 'fold3', 'fold300', 'bn_apply', 'gate_bwd', 'gate_bwd_ap']
BOUND = {'none': 2e-6, 'coef': 2e-6, 'fold1': 2e-6, 'fold3': 2e-6, 'fold300': 2e-6, 'bn_apply': 3 * 8e-6, 'gate_bwd': 3 * 4e-6, 'gate_bwd_ap': 3 * 4e-6}
# (flipped taps, statistics, bias + Dropout2d masks)
COMBOS = [(flip, stats, extras) for flip in (False, True) for stats in ('off', 'fwd', 'bwd') for extras in (True, False)]


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


def packed_weight(w):
    return w.float().permute(2, 3, 1, 0).contiguous().cuda().permute(3, 2, 0, 1)


def guarded(rows, *cols):
    return torch.full((rows + GUARD,) + cols, float('nan'), dtype=torch.float32, device='cuda')


def bits(t):
    return t.contiguous().view(torch.int32)


def act_pair(act):
    if act == 'elu':
        return F.elu, lambda u: torch.where(u > 0, torch.ones_like(u), torch.exp(u))
    return F.relu, lambda u: (u > 0).to(u.dtype)


class Case:
    """Inputs of one (shape, prologue) on the device, and the float64 input of the 3x3 convolution they amount to."""

    def __init__(self, K, shape, pro, act='elu'):
        N, H, W = shape
        self.shape, self.pro, self.act, self.M = shape, pro, act, N * H * W
        M = self.M
        g = torch.Generator().manual_seed(1000 * N + 10 * H + PROLOGUES.index(pro))
        rn = lambda *s: torch.randn(*s, generator=g)
        dev = lambda t: t.float().cuda()
        fa, fg = act_pair(act)
        self.w64 = rn(CH, CH, 3, 3).double() / 24
        self.w = packed_weight(self.w64)
        self.ge = K.ConvGeom(self.w, 1, 1)
        self.bias = dev(0.1 * rn(CH))
        self.mask = dev((torch.rand(N, CH, generator=g) < 0.8).float() / 0.8)       # Dropout2d of the epilogue
        self.pro_mask = dev((torch.rand(N, CH, generator=g) < 0.8).float() / 0.8)   # ... of a backward prologue
        self.x = dev(rn(N, H, W, CH))
        # statistics epilogue: a pivot row (forward), a coefficient block and the BatchNorm input (backward)
        self.piv = dev(0.1 * rn(CH))
        self.sblock = dev(torch.stack([0.5 + torch.rand(CH, generator=g), 0.1 * rn(CH), 0.1 * rn(CH), 0.5 + torch.rand(CH, generator=g)]))
        self.sx = dev(rn(N, H, W, CH))
        d64 = lambda t: t.double().cpu()
        x = d64(self.x)
        coef = lambda: torch.stack([0.5 + torch.rand(CH, generator=g), 0.1 * rn(CH), 0.1 * rn(CH), 0.5 + torch.rand(CH, generator=g)])

        def bn_bwd(dh, xb, block, parts):
            sc, sh, mu, rs = d64(block)
            c1, c2 = d64(parts)[:, 0].sum(0) / M, d64(parts)[:, 1].sum(0) / M
            gq = d64(dh) * fg(d64(xb) * sc + sh)
            return (gq - c1 - (d64(xb) - mu) * rs * c2) * sc

        if pro == 'none':
            h = x
        elif pro == 'coef':
            self.sc, self.sh = dev(0.5 + torch.rand(CH, generator=g)), dev(0.1 * rn(CH))
            h = fa(x * d64(self.sc) + d64(self.sh))
        elif pro.startswith('fold'):
            R = int(pro[4:])
            self.gamma, self.beta = dev(1 + 0.1 * rn(CH)), dev(0.1 * rn(CH))
            dl = x.reshape(M, CH) - d64(self.piv)
            rows = [torch.stack([c.sum(0), (c * c).sum(0)]) for c in dl.tensor_split(R)]
            self.parts = dev(torch.stack(rows + [torch.stack([d64(self.piv), torch.zeros(CH, dtype=torch.float64)])]))   # the pivot travels behind the rows
            self.R = R
            mean, var = x.mean((0, 1, 2)), x.var((0, 1, 2), unbiased=False)
            h = fa((x - mean) / torch.sqrt(var + 1e-5) * d64(self.gamma) + d64(self.beta))
        elif pro == 'bn_apply':
            self.bwd_x, self.block, self.parts = dev(rn(N, H, W, CH)), dev(coef()), dev(rn(3, 2, CH))
            h = bn_bwd(self.x, self.bwd_x, self.block, self.parts)
        else:
            self.wg64 = rn(2 * CH, CH, 1, 1).double() / 8
            self.wg = packed_weight(self.wg64)
            self.geg = K.ConvGeom(self.wg, 1, 0)
            self.ab = dev(rn(N, H, W, 2 * CH))
            go = x
            if pro == 'gate_bwd_ap':
                self.ap_x, self.ap_add, self.block, self.parts = dev(rn(N, H, W, CH)), dev(rn(N, H, W, CH)), dev(coef()), dev(rn(3, 2, CH))
                go = bn_bwd(self.x, self.ap_x, self.block, self.parts) + d64(self.ap_add)
            self.go64 = go
            a, b = d64(self.ab)[..., :CH], d64(self.ab)[..., CH:]
            s = torch.sigmoid(b)
            self.dab64 = torch.cat([go * s * fg(a), go * s * (1 - s) * fa(a)], -1)
            h = self.dab64 @ d64(self.wg).reshape(2 * CH, CH)
        self.h64 = h   # without the prologue's Dropout2d mask
        self._conv = {}

    def reference(self, flip, extras):
        """float64 y of the launch; the two 3x3 convolutions a case needs are computed once each"""
        key = (flip, extras and self.pro in ('bn_apply', 'gate_bwd', 'gate_bwd_ap'))
        if key not in self._conv:
            h = self.h64 * self.pro_mask.double().cpu()[:, None, None, :] if key[1] else self.h64
            hc = h.permute(0, 3, 1, 2)
            y = F.conv_transpose2d(hc, self.w64, padding=1) if flip else F.conv2d(hc, self.w64, padding=1)
            self._conv[key] = y.permute(0, 2, 3, 1)
        y = self._conv[key]
        if extras:
            y = (y + self.bias.double().cpu()) * self.mask.double().cpu()[:, None, None, :]
        return y


def launch(K, c, combo, nsplit):
    """One lvae_resblock_conv_f32 call on fresh NaN-filled outputs. Returns ({name: whole buffer, guards included}, rows, nsplit the plan answers)."""
    from lvae_amd import _C
    flip, stats, extras = combo
    N, H, W = c.shape
    M, pro, ptr = c.M, c.pro, K.ptr
    out = {'y': guarded(M, CH)}
    d, need = K._rb_desc(c.x, c.w, c.ge, flip, out['y'], out_scale=c.mask if extras else None)
    assert need
    d.bias = ptr(c.bias if extras else None)
    e = _C.RbExt()
    e.epilogue, e.nsplit = _C.RB_EPI_PLAIN, nsplit
    keep = None
    if pro in ('none', 'coef') or pro.startswith('fold'):
        e.prologue = _C.RB_PRO_AFFINE
        d.in_act = _C.ACT[c.act]
        if pro == 'coef':
            d.in_scale, d.in_shift = ptr(c.sc), ptr(c.sh)
        elif pro != 'none':
            out['coef'], out['rm'], out['rv'] = guarded(4, CH), torch.zeros(CH, device='cuda'), torch.ones(CH, device='cuda')
            keep = _C.BnFold(ptr(c.parts), c.R, M, ptr(c.gamma), ptr(c.beta), 1e-5, 0.1, ptr(out['rm']), ptr(out['rv']), ptr(out['coef']))
            d.in_fold = C.addressof(keep)
    elif pro == 'bn_apply':
        e.prologue = _C.RB_PRO_BN_APPLY
        out['dg'], out['db'], out['xt'] = torch.full((CH,), 0.5, device='cuda'), torch.full((CH,), -0.25, device='cuda'), guarded(M, CH)
        e.bwd_parts, e.bwd_rows, e.bwd_act, e.bwd_M = ptr(c.parts), c.parts.shape[0], _C.ACT[c.act], M
        e.bwd_coef, e.bwd_x, e.dgamma, e.dbeta, e.xt_out = ptr(c.block), ptr(c.bwd_x), ptr(out['dg']), ptr(out['db']), ptr(out['xt'])
        e.pro_drop = ptr(c.pro_mask if extras else None)
    else:
        e.prologue = _C.RB_PRO_GATE_BWD
        K._rb_gate_ws(e, c.wg, c.geg, c.x.device, True)
        out['dab'], out['xt'] = guarded(M, 2 * CH), guarded(M, CH)
        e.act, e.ab_in, e.dab, e.xt_out = _C.ACT[c.act], ptr(c.ab), ptr(out['dab']), ptr(out['xt'])
        e.pro_drop = ptr(c.pro_mask if extras else None)
        if pro == 'gate_bwd_ap':
            out['dg'], out['db'], out['ap'] = torch.full((CH,), 0.5, device='cuda'), torch.full((CH,), -0.25, device='cuda'), guarded(M, CH)
            e.ap_parts, e.ap_rows, e.ap_act, e.ap_M = ptr(c.parts), c.parts.shape[0], _C.ACT[c.act], M
            e.ap_coef, e.ap_dh, e.ap_x, e.ap_add = ptr(c.block), ptr(c.x), ptr(c.ap_x), ptr(c.ap_add)
            e.ap_dgamma, e.ap_dbeta, e.ap_out = ptr(out['dg']), ptr(out['db']), ptr(out['ap'])
        else:
            e.dout = ptr(c.x)
    lib = _C.load()
    rows = int(lib.lvae_resblock_conv_rows(C.byref(d)))
    if stats != 'off':
        out['stats'] = guarded(rows + 1, 2, CH)
        d.stats_out = ptr(out['stats'])
        if stats == 'fwd':
            d.stats_pivot = ptr(c.piv)
        else:
            d.stats_pivot, d.stats_x, d.stats_mode, d.stats_act = ptr(c.sblock), ptr(c.sx), 1, _C.ACT[c.act]
    answered = int(lib.lvae_resblock_conv_nsplit(C.byref(d), C.byref(e)))
    K.call('lvae_resblock_conv_f32', C.byref(d), C.byref(e), K.stream_ptr())
    del keep
    return out, rows, answered


def check_case(K, c, split_expected):
    N, H, W = c.shape
    M = c.M
    for combo in COMBOS:
        flip, stats, extras = combo
        one, rows, n1 = launch(K, c, combo, 1)
        two, rows2, n2 = launch(K, c, combo, 2)
        torch.cuda.synchronize()
        assert n1 == 1 and n2 == (2 if split_expected else 1) and rows == rows2 == -(-M // (64 if H * W == 64 else 32)), (combo, n1, n2, rows)
        assert sorted(one) == sorted(two)
        for name in one:   # bit for bit, guards and rows past the batch included; dgamma / dbeta and the running statistics: one increment
            assert torch.equal(bits(one[name]), bits(two[name])), (combo, name)
        for name in ('y', 'xt', 'ap', 'dab'):
            if name in two:
                assert bool(torch.isfinite(two[name][:M]).all()) and bool(torch.isnan(two[name][M:]).all()), (combo, name)
        if 'stats' in two:
            st = two['stats']   # one row per tile; forward mode: the pivot in the first half of the row behind them, nothing else
            assert bool(torch.isfinite(st[:rows]).all()) and bool(torch.isnan(st[rows, 1]).all()) and bool(torch.isnan(st[rows + 1:]).all()), combo
            assert stats == 'fwd' or bool(torch.isnan(st[rows, 0]).all()), combo
            if stats == 'fwd':
                assert torch.equal(two['stats'][rows, 0], c.piv), combo   # the pivot slot, half of it from either workgroup of tile 0
        if 'coef' in two:
            assert bool(torch.isfinite(two['coef'][:4]).all()) and bool(torch.isnan(two['coef'][4:]).all()), combo
        ref = c.reference(flip, extras)
        err = float((two['y'][:M].double().cpu().reshape(ref.shape) - ref).norm() / ref.norm())
        print('%-12s %-10s flip %d stats %-3s extras %d  y rel err %.2e (bound %.1e)' % (c.pro, c.shape, flip, stats, extras, err, BOUND[c.pro]))
        assert err < BOUND[c.pro], (combo, err)
        for name, want in (('xt', c.h64 * (c.pro_mask.double().cpu()[:, None, None, :] if extras else 1)), ('dab', getattr(c, 'dab64', None)),
                           ('ap', getattr(c, 'go64', None))):
            if name in two and want is not None:
                got = two[name][:M].double().cpu().reshape(want.shape)
                assert float((got - want).norm() / want.norm()) < BOUND[c.pro], (combo, name)


@pytest.mark.parametrize('pro', PROLOGUES)
@pytest.mark.parametrize('shape', SHAPES[:-1])
def test_split_launch_writes_what_the_unsplit_launch_writes(K, shape, pro):
    check_case(K, Case(K, shape, pro), True)


@pytest.mark.parametrize('pro', PROLOGUES)
def test_split_is_refused_on_64_pixel_tiles(K, pro):
    """8x8 images: one image is a 64-pixel tile (two 32-row blocks per wave), where the split kernel does not exist; the plan answers
    one workgroup per tile even when two are asked for, and the launch is the unsplit one."""
    check_case(K, Case(K, SHAPES[-1], pro), False)


def test_run_time_activation_build_splits_too(K):
    check_case(K, Case(K, (9, 2, 2), 'coef', act='relu'), True)
    check_case(K, Case(K, (3, 4, 4), 'gate_bwd_ap', act='relu'), True)


def test_plan_decides_by_grid_epilogue_and_precision(K):
    """nsplit = 0: two workgroups per tile while twice the tiles fit the 256 CUs, for the plain epilogue in the six-product form only."""
    from lvae_amd import _C
    lib = _C.load()
    w = packed_weight(torch.randn(CH, CH, 3, 3) / 24)
    ge = K.ConvGeom(w, 1, 1)

    def ask(N, H, epi=None, force=0):
        x = torch.zeros(N, H, H, CH, device='cuda')
        d = K._rb_query_desc(x, w, ge)
        e = _C.RbExt()
        e.epilogue, e.nsplit = _C.RB_EPI_PLAIN if epi is None else epi, force
        return int(lib.lvae_resblock_conv_nsplit(C.byref(d), C.byref(e))), int(lib.lvae_resblock_conv_rows(C.byref(d)))

    assert ask(256, 4) == (2, 128) and ask(256, 2) == (2, 32) and ask(1, 2) == (2, 1)   # the 4x4 and 2x2 levels at batch 256: 256 and 64 workgroups
    assert ask(258, 4) == (1, 129) and ask(258, 4, force=2) == (2, 129)                 # 258 workgroups: left alone unless asked for
    assert ask(512, 4) == (1, 256) and ask(600, 4, force=2) == (1, 150)                 # the grid is full; beyond it 64-pixel tiles, which never split
    assert ask(256, 8) == (1, 256) and ask(256, 8, force=2) == (1, 256)
    assert ask(256, 4, epi=_C.RB_EPI_GATE) == (1, 128) and ask(256, 4, epi=_C.RB_EPI_GATE, force=2) == (1, 128)
    assert ask(256, 4, force=1) == (1, 128)
    assert ask(256, 16) == (0, 0)
    K.set_precision('bf16')
    try:
        assert ask(256, 4) == (1, 128) and ask(256, 4, force=2) == (1, 128)
    finally:
        K.set_precision('f32')
