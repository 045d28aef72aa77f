"""Nearest-neighbour search, the parts that need no GPU: the workspace query, the argument checks of lvae_nn_l2_f32 (which come before
any launch, so they can be called with host memory), the evaluation CLI's refusals and closeness_summary."""
import ctypes

import numpy as np
import pytest
import torch

EINVAL, EALIGN, EWORKSPACE = -1, -2, -3
U8, F32 = 0, 1


@pytest.fixture(scope='module')
def lib():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    return _C.load()


def test_workspace_is_positive_and_grows_with_every_size(lib):
    ws = lib.lvae_nn_l2_workspace
    Qs = [1, 2, 31, 32, 33, 64, 65, 144, 500, 512, 513, 1000, 4096, 16384, 16385, 100000]
    Ns = [1, 2, 127, 128, 129, 1000, 1024, 1025, 4096, 50000, 65536, 65537, 1000000, 2 ** 31 - 1]
    ks = [1, 2, 7, 31, 32]
    for k in ks:
        for N in Ns:
            prev = 0
            for Q in Qs:
                w = ws(Q, N, k)
                assert w > 0 and w >= prev, (Q, N, k, w, prev)
                prev = w
        for Q in Qs:
            prev = 0
            for N in Ns:
                w = ws(Q, N, k)
                assert w >= prev, (Q, N, k, w, prev)
                prev = w
    for Q in Qs:
        for N in Ns:
            got = [ws(Q, N, k) for k in ks]
            assert got == sorted(got), (Q, N, got)
    # far below Q * N floats where the search is large: the flagship shape at the largest k
    assert ws(144, 50000, 32) < 144 * 50000 * 4 // 4
    # sizes outside the limits have no workspace
    for bad in [(0, 10, 1), (-1, 10, 1), (1, 0, 1), (1, -5, 1), (1, 2 ** 31, 1), (1, 10, 0), (1, 10, 33), (1, 10, -1)]:
        assert ws(*bad) == 0, bad


def test_refusals_return_their_code_and_touch_nothing(lib):
    Q, N, D, k = 3, 10, 5, 4
    need = lib.lvae_nn_l2_workspace(Q, N, k)
    assert need > 0
    queries = np.full((Q, D), 0.25, dtype=np.float32)
    table_u8 = np.full((N, D), 9, dtype=np.uint8)
    table_f32 = np.full((N, D), 0.5, dtype=np.float32)
    exclude = np.full((Q,), -1, dtype=np.int32)
    index = np.full((Q, k), 77, dtype=np.int32)
    dist = np.full((Q, k), 7.0, dtype=np.float32)
    ws = np.full((need + 64,), 0x5A, dtype=np.uint8)
    ws_ptr = ws.ctypes.data + (-ws.ctypes.data) % 16
    P = lambda a: None if a is None else a.ctypes.data

    def call(**change):
        a = dict(queries=P(queries), Q=Q, table=P(table_u8), kind=U8, N=N, D=D, exclude=P(exclude), k=k, index=P(index), dist=P(dist),
                 ws=ws_ptr, ws_bytes=need)
        a.update(change)
        return lib.lvae_nn_l2_f32(a['queries'], a['Q'], a['table'], a['kind'], a['N'], a['D'], a['exclude'], a['k'], a['index'], a['dist'],
                                  a['ws'], a['ws_bytes'], None)

    cases = [
        (EINVAL, dict(queries=None)), (EINVAL, dict(table=None)), (EINVAL, dict(index=None)), (EINVAL, dict(dist=None)),
        (EINVAL, dict(Q=0)), (EINVAL, dict(Q=-3)), (EINVAL, dict(N=0)), (EINVAL, dict(N=-1)), (EINVAL, dict(N=2 ** 31)),
        (EINVAL, dict(D=0)), (EINVAL, dict(D=-7)), (EINVAL, dict(k=0)), (EINVAL, dict(k=33)), (EINVAL, dict(k=-1)),
        (EINVAL, dict(kind=2)), (EINVAL, dict(kind=-1)),
        (EINVAL, dict(Q=2 ** 31 - 1, k=2)),                       # Q * k past int32
        (EINVAL, dict(N=2 ** 31 - 1, D=2 ** 40)),                 # N * D past the byte offsets
        (EINVAL, dict(table=P(table_f32), kind=F32, D=2 ** 62)),
        (EWORKSPACE, dict(ws=None)), (EWORKSPACE, dict(ws_bytes=need - 1)), (EWORKSPACE, dict(ws_bytes=0)),
        (EWORKSPACE, dict(ws=None, ws_bytes=0)),
        (EALIGN, dict(ws=ws_ptr + 4)), (EALIGN, dict(ws=ws_ptr + 1)),
    ]
    for code, change in cases:
        rc = call(**change)
        assert rc == code, (change, rc)
        assert lib.lvae_last_error(), change
    # an error in the arguments is reported before a missing workspace, a missing workspace before a misaligned one
    assert call(k=0, ws=None) == EINVAL
    assert call(ws=ws_ptr + 4, ws_bytes=need - 1) == EWORKSPACE
    assert (index == 77).all() and (dist == 7.0).all() and (ws == 0x5A).all()
    assert (queries == 0.25).all() and (table_u8 == 9).all() and (exclude == -1).all()


def test_binding_refuses_host_tensors_and_bad_shapes():
    import lvae_amd  # noqa: F401
    from lvae_amd import _C, kernels, neighbours
    with pytest.raises(_C.LvaeHipError):
        kernels.nn_l2(torch.zeros(2, 4), torch.zeros(3, 4), 1)
    with pytest.raises(_C.LvaeHipError):
        neighbours.NeighbourIndex(torch.zeros(3, 4))
    assert kernels.NN_MAX_K == 32
    sig = _C.SIGNATURES['lvae_nn_l2_f32']
    assert sig[0] is ctypes.c_int and len(sig[1]) == 13
    assert _C.load().lvae_abi_version() == _C.ABI_VERSION   # an addition: a library without the symbols fails at load


BASE = ['-d', 'cifar10', '--zdims', '8', '8', '--downsample', '1', '1', '--nfilters', '16', '--synthetic']


def _refused(argv, capsys, word):
    from lvae_amd import evaluate as leval
    with pytest.raises(SystemExit) as e:
        leval.parse_eval_args(BASE + argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_parse_eval_args_nn_flags(tmp_path, capsys):
    import lvae_amd  # noqa: F401
    from lvae_amd import evaluate as leval
    a = leval.parse_eval_args(BASE)
    assert (a.nn, a.nn_k, a.nn_space, a.nn_layers, a.nn_table) == (False, 7, 'pixel', 2, '') and a.nn_table_size >= 1
    a = leval.parse_eval_args(BASE + ['--nn', '--nn-k', '32', '--nn-space', 'latent', '--nn-layers', '1', '--nn-table-size', '50'])
    assert (a.nn, a.nn_k, a.nn_space, a.nn_layers, a.nn_table_size) == (True, 32, 'latent', 1, 50)
    _refused(['--nn', '--nn-k', '0'], capsys, '--nn-k')
    _refused(['--nn', '--nn-k', '33'], capsys, '--nn-k')
    _refused(['--nn', '--nn-k', '-2'], capsys, '--nn-k')
    _refused(['--nn', '--nn-layers', '0'], capsys, '--nn-layers')
    _refused(['--nn', '--nn-layers', '3'], capsys, '--nn-layers')
    _refused(['--nn', '--nn-space', 'cosine'], capsys, '--nn-space')
    _refused(['--nn', '--nn-table-size', '0'], capsys, '--nn-table-size')
    fits, small = str(tmp_path / 'fits.npz'), str(tmp_path / 'small.npz')
    np.savez(fits, data=np.zeros((5, 3, 32, 32), dtype=np.uint8))
    np.savez(small, data=np.zeros((5, 1, 28, 28), dtype=np.float32))
    a = leval.parse_eval_args(BASE + ['--nn', '--nn-space', 'latent', '--nn-table', fits])
    assert a.nn_table == fits
    _refused(['--nn', '--nn-space', 'latent', '--nn-table', small], capsys, '--nn-space latent')
    _refused(['--nn', '--nn-table', str(tmp_path / 'absent.npz')], capsys, '--nn-table')
    flat = str(tmp_path / 'flat.npz')
    np.savez(flat, data=np.zeros((5, 3072), dtype=np.uint8))
    _refused(['--nn', '--nn-table', flat], capsys, '--nn-table')


def test_closeness_summary_known_quantiles():
    import lvae_amd  # noqa: F401
    from lvae_amd.neighbours import closeness_line, closeness_summary
    ds = np.arange(101, dtype=np.float64)              # quantile p is 100 p
    dh = 10.0 + 2.0 * np.arange(201, dtype=np.float64)  # quantile p is 10 + 400 p: the 1 % quantile is 14
    s = closeness_summary(ds[::-1].copy(), torch.from_numpy(dh).float().view(3, 67))
    assert s['samples'] == {'median': 50.0, 'q10': 10.0, 'q90': 90.0}
    assert s['heldout'] == {'median': 210.0, 'q10': 50.0, 'q90': 370.0}
    assert s['below_heldout_q01'] == pytest.approx(14.0 / 101.0)   # samples 0 .. 13 lie strictly below 14
    assert closeness_summary([5.0], [1.0, 2.0])['below_heldout_q01'] == 0.0
    assert closeness_summary([0.0, 0.0, 9.0], [1.0, 2.0])['below_heldout_q01'] == pytest.approx(2.0 / 3.0)
    with pytest.raises(ValueError):
        closeness_summary([], [1.0])
    assert 'pixel' in closeness_line('pixel', s) and '210' in closeness_line('pixel', s)
