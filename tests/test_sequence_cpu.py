"""CPU tests of the frame-sequence surface: how a sequence is sharded over ranks, and the Python shims' argument checks,
which must reject bad input with ValueError before any device call (no GPU is needed here)."""
import numpy as np
import pytest


@pytest.mark.parametrize("world", range(1, 10))
def test_sequence_shard_covers_every_pair_once(world):
    from oflk_dist import sequence_shard

    for T in range(2, 41):
        shards = [sequence_shard(T, r, world) for r in range(world)]
        seen = [b for lo, hi in shards for b in range(lo, hi)]
        assert seen == list(range(T - 1)), (T, world, shards)
        sizes = [hi - lo for lo, hi in shards]
        assert max(sizes) - min(sizes) <= 1
        owning = [(lo, hi) for lo, hi in shards if hi > lo]
        for (lo0, hi0), (lo1, hi1) in zip(owning, owning[1:]):
            # rank r reads frames [lo, hi]: neighbours share exactly one frame
            assert set(range(lo0, hi0 + 1)) & set(range(lo1, hi1 + 1)) == {hi0}, (T, world, shards)


def test_sequence_shard_rejects_bad_arguments():
    from oflk_dist import sequence_shard

    with pytest.raises(ValueError):
        sequence_shard(1, 0, 1)
    with pytest.raises(ValueError):
        sequence_shard(5, 2, 2)
    with pytest.raises(ValueError):
        sequence_shard(5, 0, 0)


def _shims():
    import lucas_kanade_core as K
    import lucas_kanade_pyramidal as P

    return [P.lucas_kanade_pyramidal_sequence, P.lucas_kanade_pyramidal_sequence_with_log, K.lucas_kanade_single_scale_sequence]


BAD = {
    "one frame": np.zeros((1, 8, 8), np.float32),
    "no frame": [],
    "one frame in a list": [np.zeros((8, 8), np.float32)],
    "2-D array": np.zeros((8, 8), np.float32),
    "4-D array": np.zeros((3, 8, 8, 1), np.float32),
    "3-D frame in a list": [np.zeros((8, 8), np.float32), np.zeros((1, 8, 8), np.float32)],
    "mixed shapes": [np.zeros((8, 8), np.float32), np.zeros((8, 9), np.float32)],
    "mixed dtypes": [np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.float32)],
    "empty frames": np.zeros((3, 0, 8), np.float32),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_shims_reject_bad_input_before_any_device_call(what, monkeypatch):
    import _oflk

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_oflk, "lib", no_device)
    for fn in _shims():
        with pytest.raises(ValueError):
            fn(BAD[what])


def test_as_sequence_keeps_uint8_and_converts_the_rest():
    import _oflk

    a, u8 = _oflk.as_sequence([np.ones((4, 5), np.uint8)] * 3)
    assert u8 and a.dtype == np.uint8 and a.shape == (3, 4, 5) and a.flags.c_contiguous
    a, u8 = _oflk.as_sequence(np.ones((2, 4, 5), np.float64))
    assert not u8 and a.dtype == np.float32 and a.shape == (2, 4, 5)
    a, u8 = _oflk.as_sequence(np.ones((6, 4, 5), np.uint8)[::2])
    assert u8 and a.shape == (3, 4, 5) and a.flags.c_contiguous
