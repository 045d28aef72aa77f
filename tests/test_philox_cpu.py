"""oracle/philox_ref.py, the CPU restatement of the device noise generator, against the published Philox4x32-10 known answers."""
import numpy as np

from oracle import philox_ref as P


def _hex(words):
    return ' '.join('%08x' % int(w) for w in words)


def test_philox4x32_10_known_answers():
    kat = [
        ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1'),
    ]
    for ctr, key, want in kat:
        assert _hex([w[0] for w in P.philox4x32_10(ctr, key)]) == want
    # the three blocks at once: the restatement is elementwise over arrays of counters (one key)
    out = P.philox4x32_10(([0, 1, 2], 0, 5, 9), (3, 4))
    for i in range(3):
        assert [int(w[i]) for w in out] == [int(w[0]) for w in P.philox4x32_10((i, 0, 5, 9), (3, 4))]


def test_counter_layout():
    # element i is word i % 4 of block i // 4; stream id and step go into counter words 2 and 3, their high halves into the key
    seed, off, sid = (1 << 40) + 77, (1 << 32) + 5, (1 << 32) + 3
    r = P.raw_words(11, seed, off, sid)
    key = seed ^ (off >> 32 << 32) ^ (sid >> 32)
    for blk in range(3):
        want = [int(w[0]) for w in P.philox4x32_10((blk, 0, 3, 5), (key & 0xffffffff, key >> 32))]
        assert [int(v) for v in r[4 * blk:4 * blk + 4]] == want[:len(r[4 * blk:4 * blk + 4])]
    assert not np.array_equal(P.raw_words(8, seed, off, sid), P.raw_words(8, seed, off + 1, sid))
    assert not np.array_equal(P.raw_words(8, seed, off, sid), P.raw_words(8, seed, off, sid + 1))


def test_u01_range_and_the_rounding_tie_at_the_top():
    edge = np.array([0, 0xff, 0x100, 0x7fffffff, 0xfffffe00, 0xffffff00, 0xffffffff], dtype=np.uint32)
    u = P.u01(edge)
    assert u.dtype == np.float32
    assert float(u[0]) == 2.0 ** -25 and float(u[1]) == 2.0 ** -25 and float(u[2]) == 1.5 * 2.0 ** -24
    # without the clamp the top input rounds to exactly 1: 16777215.5 is a tie in fp32
    top = (np.float32(0xffffff) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert float(top) == 1.0
    assert float(u[-1]) == float(u[-2]) == 1.0 - 2.0 ** -24 and float(u.max()) < 1.0
    # every other input is untouched by the clamp
    rest = np.arange(0xffffff - 4096, 0xffffff, dtype=np.uint32) << np.uint32(8)
    unclamped = ((rest >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert np.array_equal(P.u01(rest), unclamped) and float(unclamped.max()) < 1.0


def test_the_draw_that_used_to_round_to_one():
    """seed 4, stream id 1, step 0: flat element 2170657 (block 542664, word 1) has its top 24 bits set, so u01 without the clamp is
    exactly 1.0, uniform(0, 1) returned 1 and a keep-probability of 1.0 dropped the element (tests/test_elementwise_gpu.py runs it)."""
    r = P.raw_words(2170660, 4, 0, 1)
    assert 2170657 // 4 == 542664 and 2170657 % 4 == 1
    assert int(r[2170657]) >> 8 == 0xffffff
    assert int((r >> np.uint32(8) == 0xffffff).sum()) == 1       # the only such draw of this fill
    u = P.uniform(r, 0.0, 1.0)
    assert 0.0 < float(u.min()) and float(u.max()) == 1.0 - 2.0 ** -24 < 1.0
    assert float(P.keep_drop(r, 1.0, 1.0).min()) == 1.0


def test_output_maps():
    r = P.raw_words(4099, 1234, 7, 2)
    u = P.uniform(r, 1e-5, 1 - 1e-5)
    assert u.dtype == np.float32 and 0 < float(u.min()) and float(u.max()) < 1 and abs(float(u.mean()) - 0.5) < 0.02
    k = P.keep_drop(r, 0.8, 1.25)
    assert set(np.unique(k).tolist()) == {0.0, 1.25} and abs(float((k > 0).mean()) - 0.8) < 0.03
    z = P.fill(4099, 'normal', 0, 0, 1234, 7, 2)
    assert z.shape == (4099,) and abs(float(z.mean())) < 0.06 and abs(float(z.std()) - 1) < 0.05
    assert np.array_equal(P.fill(4099, 'uniform', 1e-5, 1 - 1e-5, 1234, 7, 2), u)
    assert np.array_equal(P.fill(5, 'normal', 0, 0, 1234, 7, 2), z[:5])      # a ragged tail is cut from a whole block
