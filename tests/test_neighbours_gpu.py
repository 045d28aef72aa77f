"""Exact nearest-neighbour search on the device (csrc/neighbours.hip, kernels.nn_l2, neighbours.py, evaluate --nn).

The reference is float64 on the CPU, written here: d64[q, n] = sum_i (q_i - t_i)^2 with a uint8 element meaning v / 255. Distances follow
the project's element-wise rule, |kernel - r64| <= 2 max|r32 - r64| + 1e-5 |r64| + 1e-6, where r32 is (q - t).pow(2).sum(-1) in float32 on
the CPU; every comparison prints `yardstick | case | kernel error | r32 error | bound` before it asserts (run with -s). Everything else
(order, ties, exclusion, independence of the launch cut, capture) is exact."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

INF, NAN = float('inf'), float('nan')
QS, NS, DS, KINDS = (1, 5, 33), (1, 7, 257, 1031), (1, 3, 17, 784, 3075), ('u8', 'f32')
QMAX = max(QS)


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


def as_f64(table):
    return table.double() / 255.0 if table.dtype == torch.uint8 else table.double()


def as_f32(table):
    return table.float().div_(255.0) if table.dtype == torch.uint8 else table


def dist64(queries, table):
    """(Q, N) float64, one query at a time (a (Q, N, D) difference would not fit)"""
    t = as_f64(table)
    return torch.stack([(t - q.double()).pow(2).sum(-1) for q in queries])


def dist32(queries, table):
    t = as_f32(table)
    return torch.stack([(q - t).pow(2).sum(-1) for q in queries])


def make(kind, N, D, Q, seed):
    """a table and queries on the CPU; every third query is a table row plus a small step, the near-duplicate the search exists for"""
    gen = torch.Generator().manual_seed(seed)
    if kind == 'u8':
        table = torch.randint(0, 256, (N, D), dtype=torch.uint8, generator=gen)
        queries = torch.rand((Q, D), generator=gen)
    else:
        table = torch.randn((N, D), generator=gen)
        queries = torch.randn((Q, D), generator=gen)
    for q in range(0, Q, 3):
        queries[q] = as_f32(table[(7 * q) % N].clone()) + 1e-3 * torch.randn(D, generator=gen)
    return table, queries


_cases = {}


def case(kind, N, D):
    """table, QMAX queries, d64 (QMAX, N), r32 error: computed once per (kind, N, D); smaller Q take the first rows"""
    key = (kind, N, D)
    if key not in _cases:
        table, queries = make(kind, N, D, QMAX, 1000 * N + D)
        d64 = dist64(queries, table)
        e32 = (dist32(queries, table).double() - d64).abs()
        _cases[key] = (table, queries, d64, e32, table.cuda(), queries.cuda())
    return _cases[key]


_runs = {}


def run(K, kind, N, D, Q):
    key = (kind, N, D, Q)
    if key not in _runs:
        _, _, _, _, tg, qg = case(kind, N, D)
        index, dist = K.nn_l2(qg[:Q].contiguous(), tg, min(N, 5))
        _runs[key] = (index.cpu().long(), dist.cpu())
    return _runs[key]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. distances and 2. ranking, over every shape
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('kind', KINDS)
def test_distances_follow_the_elementwise_rule(K, kind, N, D):
    _, _, d64, e32, _, _ = case(kind, N, D)
    for Q in QS:
        index, dist = run(K, kind, N, D, Q)
        k = min(N, 5)
        assert index.shape == dist.shape == (Q, k)
        assert bool(((index >= 0) & (index < N)).all()), (kind, Q, N, D)
        r64 = d64[:Q].gather(1, index)
        worst32 = float(e32[:Q].max())
        bound = 2.0 * worst32 + 1e-5 * r64.abs() + 1e-6
        err = (dist.double() - r64).abs()
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, INF))
        j = int(torch.argmax(err / bound))
        print('yardstick | %-40s | kernel %.3e | r32 %.3e | bound %.3e | n %d'
              % ('nn_l2 %s Q %d N %d D %d' % (kind, Q, N, D), float(err.flatten()[j]), worst32, float(bound.flatten()[j]), err.numel()))
        assert bool((err <= bound).all()), (kind, Q, N, D, float(err.flatten()[j]), float(bound.flatten()[j]))


@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('kind', KINDS)
def test_ranking(K, kind, N, D):
    _, _, d64, e32, _, _ = case(kind, N, D)
    for Q in QS:
        index, dist = run(K, kind, N, D, Q)
        k = min(N, 5)
        got = d64[:Q].gather(1, index)
        best = d64[:Q].sort(1).values[:, :k]
        bound = 2.0 * float(e32[:Q].max()) + 1e-5 * best.abs() + 1e-6
        over = got - best
        j = int(torch.argmax(over / bound))
        print('yardstick | %-40s | kernel %.3e | r32 %.3e | bound %.3e | n %d'
              % ('nn_l2 rank %s Q %d N %d D %d' % (kind, Q, N, D), float(over.flatten()[j]), float(e32[:Q].max()), float(bound.flatten()[j]),
                 over.numel()))
        assert bool((over <= bound).all()), (kind, Q, N, D)
        for q in range(Q):
            keys = [(float(dist[q, r]), int(index[q, r])) for r in range(k)]
            assert all(a < b for a, b in zip(keys, keys[1:])), (kind, Q, N, D, q, keys)   # strictly increasing (distance, row)
            assert len(set(i for _, i in keys)) == k


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. exact cases
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Q,N,D,k', [(9, 300, 1024, 32), (4, 40, 5, 32), (33, 700, 3, 7), (2100, 3000, 4, 32)])
def test_small_integers_sort_exactly(K, Q, N, D, k):
    """values 0..3: every sum is exact in fp32 and ties abound. (2100, 3000): more query tiles than row groups, so a workgroup merges
    several slabs into its running list."""
    gen = torch.Generator().manual_seed(Q + N)
    table = torch.randint(0, 4, (N, D), generator=gen).float()
    queries = torch.randint(0, 4, (Q, D), generator=gen).float()
    index, dist = K.nn_l2(queries.cuda(), table.cuda(), k)
    d = torch.cat([dist64(queries[lo:lo + 256], table) for lo in range(0, Q, 256)])
    order = d.sort(dim=1, stable=True)
    kk = min(k, N)
    assert torch.equal(index.cpu().long()[:, :kk], order.indices[:, :kk])
    assert same_bits(dist.cpu()[:, :kk], order.values[:, :kk].float())
    if kk < k:
        assert bool((index.cpu()[:, kk:] == -1).all()) and bool((dist.cpu()[:, kk:] == INF).all())


def test_a_query_equal_to_a_row_is_at_distance_zero(K):
    gen = torch.Generator().manual_seed(4)
    N, D = 400, 3075
    table = torch.randint(0, 256, (N, D), dtype=torch.uint8, generator=gen)
    table[300] = table[20]     # duplicated rows: the lower one is returned
    table[399] = table[131]
    rows = [0, 20, 300, 131, 399, 128, 255, 7]
    queries = table[rows].float() / 255
    index, dist = K.nn_l2(queries.cuda(), table.cuda(), 2)
    index, dist = index.cpu(), dist.cpu()
    assert index[:, 0].tolist() == [0, 20, 20, 131, 131, 128, 255, 7]
    assert bool((bits(dist[:, 0]) == 0).all())          # +0.0f exactly
    assert index[1:5, 1].tolist() == [300, 300, 399, 399] and bool((bits(dist[1:5, 1]) == 0).all())
    tf = torch.randn((50, 17), generator=gen)
    index, dist = K.nn_l2(tf[[49, 3]].contiguous().cuda(), tf.cuda(), 1)
    assert index.cpu().flatten().tolist() == [49, 3] and bool((bits(dist.cpu()) == 0).all())


def test_identical_rows_come_back_in_row_order(K):
    table = torch.full((5000, 4), 0.375)
    index, dist = K.nn_l2(torch.tensor([[0.5, 0.25, 0.375, 1.0]]).cuda(), table.cuda(), 32)
    assert index.cpu().flatten().tolist() == list(range(32))
    assert bool((dist.cpu() == dist.cpu()[0, 0]).all())
    tb = torch.full((5000, 4), 9, dtype=torch.uint8)
    index, _ = K.nn_l2(torch.rand(3, 4).cuda(), tb.cuda(), 32)
    assert index.cpu().tolist() == [list(range(32))] * 3


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. a pair's bits do not depend on the rest of the call
# ---------------------------------------------------------------------------------------------------------------------------------
def pairs(index, dist):
    return [{int(i): int(b) for i, b in zip(index[q].tolist(), bits(dist[q]).tolist()) if i >= 0} for q in range(index.shape[0])]


@pytest.mark.parametrize('kind', KINDS)
def test_one_query_alone_and_inside_a_batch(K, kind):
    table, queries = make(kind, 600, 3075, 33, 11)
    tg = table.cuda()
    ib, db = K.nn_l2(queries.cuda(), tg, 32)
    for q in (0, 13, 32):
        i1, d1 = K.nn_l2(queries[q:q + 1].cuda(), tg, 32)
        assert torch.equal(i1[0], ib[q]) and same_bits(d1[0], db[q]), (kind, q)


@pytest.mark.parametrize('kind', KINDS)
def test_a_table_and_its_sub_range(K, kind):
    a, b = 37, 291
    table, queries = make(kind, 300, 3075, 5, 12)
    tg = table.cuda()
    i_full, d_full = K.nn_l2(queries.cuda(), tg, 32)
    i_sub, d_sub = K.nn_l2(queries.cuda(), tg[a:b], 32)       # rows at an odd offset: another alignment, another cut into slabs
    i_full, d_full, i_sub, d_sub = i_full.cpu(), d_full.cpu(), i_sub.cpu(), d_sub.cpu()
    for q in range(5):
        inside = [(int(i), int(v)) for i, v in zip(i_full[q].tolist(), bits(d_full[q]).tolist()) if a <= i < b]
        assert len(inside) > 0
        sub = [(int(i) + a, int(v)) for i, v in zip(i_sub[q].tolist(), bits(d_sub[q]).tolist())]
        assert sub[:len(inside)] == inside, (kind, q)         # what the full search found inside [a, b) leads the sub-range's list
    # every pair of a short sub-range, against the same rows found one at a time in the full table
    i_all, d_all = K.nn_l2(queries.cuda(), tg[a:a + 31], 31)
    for q in range(5):
        want = pairs(*[t.cpu() for t in K.nn_l2(queries[q:q + 1].cuda(), tg[:a + 31], 32)])[0]
        got = pairs(i_all.cpu(), d_all.cpu())[q]
        shared = [i for i in got if i + a in want]
        assert shared and all(got[i] == want[i + a] for i in shared), (kind, q)


@pytest.mark.parametrize('kind', KINDS)
def test_k_and_exclude_change_no_distance(K, kind):
    table, queries = make(kind, 1031, 784, 33, 13)
    tg, qg = table.cuda(), queries.cuda()
    i32_, d32_ = K.nn_l2(qg, tg, 32)
    i1, d1 = K.nn_l2(qg, tg, 1)
    assert torch.equal(i1[:, 0], i32_[:, 0]) and same_bits(d1[:, 0], d32_[:, 0])
    i7, d7 = K.nn_l2(qg, tg, 7)
    assert torch.equal(i7, i32_[:, :7]) and same_bits(d7, d32_[:, :7])
    ex = i32_[:, 3].clone().contiguous()                       # skip what was fourth
    ie, de = K.nn_l2(qg, tg, 31, exclude=ex)
    keep = [0, 1, 2] + list(range(4, 32))
    assert torch.equal(ie, i32_[:, keep]) and same_bits(de, d32_[:, keep])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. exclude
# ---------------------------------------------------------------------------------------------------------------------------------
def test_exclude(K):
    gen = torch.Generator().manual_seed(21)
    N, D, Q, k = 300, 17, 33, 9
    table = torch.randint(0, 256, (N, D), dtype=torch.uint8, generator=gen)
    rows = torch.randint(0, N, (Q,), generator=gen)
    queries = table[rows].float() / 255                        # every query is a table row: its own nearest neighbour
    tg, qg = table.cuda(), queries.cuda()
    ip, dp = K.nn_l2(qg, tg, k + 1)
    assert bool((dp[:, 0] == 0).all())
    own = ip[:, 0].clone().contiguous()
    ie, de = K.nn_l2(qg, tg, k, exclude=own)
    assert not bool((ie == own[:, None]).any())                # the excluded row never appears
    assert torch.equal(ie, ip[:, 1:]) and same_bits(de, dp[:, 1:])   # every other row keeps its place
    # all -1 is the plain call
    im, dm = K.nn_l2(qg, tg, k + 1, exclude=torch.full((Q,), -1, dtype=torch.int32).cuda())
    assert torch.equal(im, ip) and same_bits(dm, dp)
    # entries outside [-1, N) skip nothing
    wild = torch.tensor([N, N + 1, 2 ** 31 - 1, -2, -(2 ** 31), N + 127, N + 128, -1000] * 5, dtype=torch.int32)[:Q].contiguous()
    iw, dw = K.nn_l2(qg, tg, k + 1, exclude=wild.cuda())
    assert torch.equal(iw, ip) and same_bits(dw, dp)
    # k = N with one exclusion ends in (-1, +inf)
    small, sq = tg[:12].contiguous(), qg[:5].contiguous()
    ia, da = K.nn_l2(sq, small, 12)
    ex = torch.tensor([0, 11, 5, -1, 3], dtype=torch.int32).cuda()
    ib, db = K.nn_l2(sq, small, 12, exclude=ex)
    ia, da, ib, db = ia.cpu(), da.cpu(), ib.cpu(), db.cpu()
    for q, e in enumerate(ex.cpu().tolist()):
        if e < 0:
            assert torch.equal(ib[q], ia[q]) and same_bits(db[q], da[q])
            continue
        keep = [j for j in range(12) if int(ia[q, j]) != e]
        assert torch.equal(ib[q, :11], ia[q, keep]) and same_bits(db[q, :11], da[q, keep])
        assert int(ib[q, 11]) == -1 and float(db[q, 11]) == INF
    # a one-row table whose row is excluded: nothing is eligible
    i0, d0 = K.nn_l2(sq, small[:1], 3, exclude=torch.zeros(5, dtype=torch.int32).cuda())
    assert bool((i0 == -1).all()) and bool((d0 == INF).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. special values
# ---------------------------------------------------------------------------------------------------------------------------------
def test_special_values(K):
    gen = torch.Generator().manual_seed(31)
    N, D = 200, 17
    table = torch.randn((N, D), generator=gen)
    table[5, 3] = NAN
    table[150, 0] = NAN
    table[9, 16] = INF
    table[140, 2] = -INF
    queries = torch.randn((4, D), generator=gen)
    index, dist = K.nn_l2(queries.cuda(), table.cuda(), 32)
    assert not bool(torch.isin(index.cpu(), torch.tensor([5, 150, 9, 140])).any())
    assert bool(torch.isfinite(dist.cpu()).all())
    small = table[[5, 9, 150, 140, 0, 1, 2]].contiguous()      # rows: NaN, inf, NaN, inf, three finite
    index, dist = K.nn_l2(queries.cuda(), small.cuda(), 7)
    index, dist = index.cpu(), dist.cpu()
    d64 = dist64(queries, small)
    for q in range(4):
        finite = sorted([4, 5, 6], key=lambda j: (float(d64[q, j]), j))
        assert index[q].tolist() == finite + [1, 3, 0, 2]         # finite, then +inf by row, then NaN by row
        assert bool(torch.isfinite(dist[q, :3]).all()) and dist[q, 3:5].tolist() == [INF, INF] and bool(torch.isnan(dist[q, 5:]).all())
    # a NaN query: every distance is NaN, the order is the row order
    queries[2, 4] = NAN
    index, dist = K.nn_l2(queries.cuda(), table.cuda(), 6)
    assert index.cpu()[2].tolist() == list(range(6)) and bool(torch.isnan(dist.cpu()[2]).all())
    assert bool(torch.isfinite(dist.cpu()[[0, 1, 3]]).all())
    tb = torch.randint(0, 256, (300, 5), dtype=torch.uint8, generator=gen)
    index, dist = K.nn_l2(torch.full((1, 5), NAN).cuda(), tb.cuda(), 32)
    assert index.cpu()[0].tolist() == list(range(32)) and bool(torch.isnan(dist.cpu()).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. capture
# ---------------------------------------------------------------------------------------------------------------------------------
def test_captured_call_replays_on_new_inputs(K):
    gen = torch.Generator().manual_seed(41)
    N, D, Q, k = 700, 48, 9, 6
    tables = [torch.randint(0, 256, (N, D), dtype=torch.uint8, generator=gen) for _ in range(3)]
    queries = [torch.rand((Q, D), generator=gen) for _ in range(3)]
    excl = [torch.randint(-1, N, (Q,), generator=gen).to(torch.int32) for _ in range(3)]
    tg, qg, eg = tables[0].cuda(), queries[0].cuda(), excl[0].cuda()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        K.nn_l2(qg, tg, k, exclude=eg)                            # the stream's scratch buffer exists before the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode='thread_local'):
            index, dist = K.nn_l2(qg, tg, k, exclude=eg)
        for j in (1, 2):
            tg.copy_(tables[j]), qg.copy_(queries[j]), eg.copy_(excl[j])
            graph.replay()
            torch.cuda.synchronize()
            got_i, got_d = index.clone(), dist.clone()
            want_i, want_d = K.nn_l2(qg, tg, k, exclude=eg)
            assert torch.equal(got_i, want_i) and same_bits(got_d, want_d), j
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. NeighbourIndex
# ---------------------------------------------------------------------------------------------------------------------------------
def test_neighbour_index(K):
    from lvae_amd.data import DeviceDataset
    from lvae_amd.neighbours import NeighbourIndex
    gen = torch.Generator().manual_seed(51)
    N, C, H, W = 90, 3, 8, 6
    chw = torch.randint(0, 256, (N, C, H, W), dtype=torch.uint8, generator=gen)
    hwc = chw.permute(0, 2, 3, 1).contiguous()
    ds = DeviceDataset(chw, None, seed=1)
    ix = NeighbourIndex.from_dataset(ds)
    assert ix.table.data_ptr() == ds.table.data_ptr() and ix.table.dtype == torch.uint8 and not ix.channels_last
    ds_last = DeviceDataset(hwc, None, seed=1, channels_last=True)
    ix_last = NeighbourIndex.from_dataset(ds_last)
    assert ix_last.table.data_ptr() == ds_last.table.data_ptr() and ix_last.channels_last and ix_last.chw == (C, H, W)
    x = (chw[[3, 77, 14]].float() / 255 + 0.01 * torch.rand((3, C, H, W), generator=gen)).cuda()
    x = torch.cat((x, torch.rand((20, C, H, W), generator=gen).cuda()))
    i_a, d_a = ix.query(x, k=5)
    i_b, d_b = ix_last.query(x, k=5)
    assert i_a.dtype == torch.int64 and d_a.dtype == torch.float32 and i_a.shape == d_a.shape == (23, 5)
    assert i_a[:3, 0].tolist() == [3, 77, 14]
    assert torch.equal(i_a, i_b)                                  # the same images in either layout (the sums run in another order)
    # rows in, rows out; (Q, D) rows are taken as they are
    i_r, d_r = ix.query(x.reshape(23, -1), k=5)
    assert torch.equal(i_r, i_a) and same_bits(d_r, d_a)
    # cut into calls of 7: the same bits
    ex = torch.tensor([3, 77] + [-1] * 21)
    i_1, d_1 = ix.query(x, k=5, exclude=ex)
    i_7, d_7 = ix.query(x, k=5, exclude=ex, max_rows=7)
    assert torch.equal(i_1, i_7) and same_bits(d_1, d_7)
    assert 3 not in i_1[0].tolist() and 77 not in i_1[1].tolist() and torch.equal(i_1[2:], i_a[2:])
    # the rows behind an index, -1 as zeros, in the layout of the queries
    idx = torch.tensor([[0, 89, -1], [5, 5, 44]]).cuda()
    want = chw.float().div(255)[idx.cpu().clamp(min=0)]
    want[0, 2] = 0
    for index_obj in (ix, ix_last):
        got = index_obj.rows(idx)
        assert got.shape == (2, 3, C, H, W) and got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    # feature rows
    feats = torch.randn((40, 11), generator=gen).cuda()
    fx = NeighbourIndex(feats)
    i_f, d_f = fx.query(feats[[7, 30]], k=1)
    assert i_f.flatten().tolist() == [7, 30] and bool((d_f == 0).all())
    assert torch.equal(fx.rows(torch.tensor([30, -1])).cpu(), torch.stack((feats[30].cpu(), torch.zeros(11))))
    with pytest.raises(ValueError):
        ix.query(torch.zeros(2, 3, 8, 7).cuda())
    with pytest.raises(ValueError):
        ix.query(x, k=33)
    with pytest.raises(ValueError):
        ix.query(x, exclude=torch.zeros(5))


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. latent features
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gauss():
    import lvae_amd  # noqa: F401
    from lvae_amd.models.lvae import LadderVAE
    g = load_golden('tiny_gauss')   # two layers, 3 x 16 x 16
    torch.manual_seed(0)
    m = LadderVAE(**g.cfg)
    m.load_state_dict(g.state_dict(), strict=True)
    m.cuda().eval()
    images = torch.floor(256 * torch.rand((22, 3, 16, 16), generator=torch.Generator().manual_seed(61))) / 255
    return m, images


@pytest.mark.parametrize('k', [1, 2])
def test_latent_features_are_the_flattened_encode(gauss, k):
    from lvae_amd.neighbours import latent_features
    m, images = gauss
    m.train()                                                    # the call switches to eval mode and back
    feats = latent_features(m, images, k, batch_size=8)
    assert m.training
    m.eval()
    want = []
    for lo in range(0, 22, 8):
        z = m.encode(images[lo:lo + 8].cuda(), k)
        assert [t is not None for t in z] == [i >= 2 - k for i in range(2)]
        want.append(torch.cat([z[i].reshape(z[i].shape[0], -1) for i in (1, 0)[:k]], 1))
    want = torch.cat(want)
    assert feats.dtype == torch.float32 and feats.shape == want.shape and feats.is_cuda
    assert same_bits(feats.cpu(), want.cpu())


def test_latent_neighbours_of_the_table_itself(gauss):
    from lvae_amd.neighbours import NeighbourIndex, latent_features
    m, images = gauss
    feats = latent_features(m, images, 2, batch_size=8)
    ix = NeighbourIndex(feats)
    q = latent_features(m, images, 2, batch_size=8)
    index, dist = ix.query(q, k=2)
    assert index[:, 0].tolist() == list(range(22)) and bool((dist[:, 0] == 0).all())
    other, d_other = ix.query(q, k=1, exclude=torch.arange(22))
    assert torch.equal(other[:, 0], index[:, 1]) and same_bits(d_other[:, 0], dist[:, 1])
    assert bool((other[:, 0] != torch.arange(22).cuda()).all()) and bool((d_other > 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. the evaluation CLI
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('space', ['pixel', 'latent'])
def test_nn_cli(tmp_path, monkeypatch, capsys, space):
    import lvae_amd  # noqa: F401
    from lvae_amd import evaluate as leval
    from lvae_amd.images import grid_shape
    from test_images_cpu import decode_png
    monkeypatch.chdir(tmp_path)
    img_dir = str(tmp_path / 'pics')
    gen = torch.Generator().manual_seed(71)
    data = torch.floor(256 * torch.rand((16, 3, 32, 32), generator=torch.Generator().manual_seed(3))) / 255   # main.synthetic_batch
    table = torch.randint(0, 256, (150, 3, 32, 32), dtype=torch.uint8, generator=gen)
    table[100] = (data[2] * 255).round().to(torch.uint8)          # an evaluation image sits in the table
    np.savez(str(tmp_path / 'table.npz'), data=table.numpy())
    argv = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--skip', '--gated',
            '--freebits', '1.0', '--batch-size', '8', '--synthetic', '--seed', '3', '--n-test', '16']
    leval.main(argv + ['--nn', '--nn-k', '3', '--nn-space', space, '--nn-table', 'table.npz', '--img-dir', img_dir])
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('nn %s:' % space)]
    assert len(line) == 1 and 'held-out median' in line[0]
    tf = table.float().div(255).numpy()
    for name, n in (('samples', 12), ('heldout', 12)):
        stem = str(tmp_path / ('nn_%s_%s' % (space, name)))
        rows, index, dist = np.load(stem + '.npy'), np.load(stem + '_index.npy'), np.load(stem + '_dist.npy')
        assert rows.shape == (n, 4, 3, 32, 32) and rows.dtype == np.float32
        assert index.shape == (n, 3) and dist.shape == (n, 3) and dist.dtype == np.float32
        assert index.min() >= 0 and index.max() < 150 and (np.diff(dist, axis=1) >= 0).all()
        for j in range(3):
            assert np.array_equal(rows[:, 1 + j], tf[index[:, j]]), (name, j)   # column j is table row index[:, j - 1]
        if name == 'heldout':
            assert np.array_equal(rows[:, 0], data[:12].numpy())                 # column 0 is the query
            assert index[2, 0] == 100 and (space != 'pixel' or dist[2, 0] == 0.0)
        png = decode_png(open(os.path.join(img_dir, 'nn_%s_%s.png' % (space, name)), 'rb').read())
        assert png.shape == tuple(grid_shape(n * 4, 4, 32, 32)) + (3,)
    # the table made up by the run itself
    leval.main(argv + ['--nn', '--nn-k', '2', '--nn-space', space, '--nn-table-size', '40'])
    assert np.load(str(tmp_path / ('nn_%s_samples.npy' % space))).shape == (12, 3, 3, 32, 32)
    assert np.load(str(tmp_path / ('nn_%s_heldout_index.npy' % space))).max() < 40
