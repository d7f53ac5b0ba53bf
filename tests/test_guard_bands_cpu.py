"""The guard-band helper held to its purpose, without a GPU (python -m pytest tests/test_guard_bands_cpu.py -q).

CPU "kernels" that misbehave in a known way write through a guarded buffer; each must be reported with the right side and
offsets under the two-fill rule, and a correct one must pass.  The layout is asserted, and the coverage table of
tests/guard_bands.py is held to include/oflk.h: a device entry point added later fails here until it is placed.
"""
import re

import numpy as np
import pytest

import guard_bands as GB

H, W, F = 5, 9, 3          # a float32 [F][H][W] output
ROW, FRAME = 4 * W, 4 * W * H
NB = F * FRAME


def _mem(g):
    """the allocation as a NumPy array that shares its memory, and the payload's offset in it"""
    return g.raw.numpy(), g.start


def _correct(g):
    m, s = _mem(g)
    m[s:s + g.nbytes] = 1


def _writer(lo, hi, value=0xEE):
    """writes the payload, and `value` at the bytes [lo, hi) relative to the payload's start"""
    def run(g):
        m, s = _mem(g)
        m[s:s + g.nbytes] = 1
        m[s + lo:s + hi] = value
    return run


BAD = {  # name: (writer, side, first, last) in the offsets of the message
    "one byte behind": (_writer(NB, NB + 1), "BEHIND", 0, 0),
    "one byte ahead": (_writer(-1, 0), "AHEAD", -1, -1),
    "a 16-byte store across the end": (_writer(NB - 4, NB + 12), "BEHIND", 0, 11),
    "a 16-byte store across the start": (_writer(-12, 4), "AHEAD", -12, -1),
    "a whole extra row": (_writer(NB, NB + ROW), "BEHIND", 0, ROW - 1),
    "a whole extra frame": (_writer(NB, NB + FRAME), "BEHIND", 0, FRAME - 1),
    "a frame one slot early": (_writer(-FRAME, 0), "AHEAD", -FRAME, -1),
}


def _run_both(writer, **kw):
    """the two-fill rule: the messages of the two runs (None where a run is clean)"""
    msgs = []
    for fill in GB.FILLS:
        g = GB.guarded(NB, fill=fill, row_bytes=ROW, name="out", **kw)
        writer(g)
        try:
            g.check("cpu writer")
            msgs.append(None)
        except AssertionError as e:
            msgs.append(str(e))
    return msgs


@pytest.mark.parametrize("skew", [0, 1, 4])
@pytest.mark.parametrize("name", list(BAD))
def test_a_writer_that_strays_is_reported_with_side_and_offsets(name, skew):
    writer, side, first, last = BAD[name]
    for msg in _run_both(writer, skew=skew):
        assert msg is not None, f"{name}: not noticed"
        assert msg.startswith("out (cpu writer)") and side in msg and f"offsets {first} .. {last} " in msg, msg


@pytest.mark.parametrize("skew", [0, 1, 2, 4])
def test_a_correct_writer_passes(skew):
    assert _run_both(_correct, skew=skew) == [None, None]
    for fill in GB.FILLS:
        g = GB.guarded(NB, fill=fill, skew=skew)
        _correct(g)
        g.check()
        assert (g.numpy() == 1).all()


@pytest.mark.parametrize("side,off", [("back", 0), ("back", 7), ("front", -1), ("front", -300)])
def test_a_constant_that_equals_one_fills_pattern_byte_is_caught_by_the_other_fill(side, off):
    probe = GB.guarded(NB, fill=GB.FILLS[0])
    value = probe.band_byte(side, off)                      # what fill 0 holds at that position
    at = NB + off if side == "back" else off
    msgs = _run_both(_writer(at, at + 1, value))
    assert msgs[0] is None, "the stray byte equals the first fill's pattern there: that run cannot see it"
    assert msgs[1] is not None and f"offsets {off} .. {off} " in msgs[1], msgs
    # and a constant over a stretch of a band is seen under either fill: the pattern is not a constant
    lo = NB if side == "back" else -64
    for msg in _run_both(_writer(lo, lo + 64, value)):
        assert msg is not None


def test_the_two_fills_differ_in_every_byte_and_neither_is_a_constant():
    o = np.arange(-70000, 70000)
    a, b = GB.pattern(o, GB.FILLS[0]), GB.pattern(o, GB.FILLS[1])
    assert ((a ^ b) == 0xFF).all()
    assert len(np.unique(a)) == 256 and (a[1:] != a[:-1]).all(), "neighbouring bytes differ"
    for k in (4, 16, 256, ROW, FRAME):                      # no period a strided copy of the band could hide behind
        assert (a[k:] != a[:-k]).mean() > 0.9, k


@pytest.mark.parametrize("align,skew", [(256, 0), (256, 1), (256, 2), (256, 4), (256, 255), (4096, 0), (4096, 12), (16, 8)])
@pytest.mark.parametrize("nbytes", [1, 3, 180, NB, 5000, 200000])
def test_the_layout(nbytes, align, skew):
    for row_bytes in (None, 36, 4096):
        g = GB.guarded(nbytes, align=align, skew=skew, row_bytes=row_bytes)
        base = g.raw.data_ptr()
        assert g.ptr == base + g.start and (g.ptr - skew) % align == 0
        if skew:
            assert g.ptr % align == skew
        want = max(4096, nbytes if row_bytes is None else min(16 * row_bytes, nbytes))
        assert g.band == want == GB.band_bytes(nbytes, row_bytes)
        assert g.front >= g.band and g.back == g.band
        assert g.end == g.start + nbytes and g.raw.numel() == g.end + g.back, "no byte between the payload and the back band"
        m = g.raw.numpy()
        assert np.array_equal(m[:g.start], GB.pattern(np.arange(-g.front, 0), g.fill)), "the front band ends at the payload"
        assert np.array_equal(m[g.end:], GB.pattern(np.arange(nbytes, nbytes + g.back), g.fill))
        assert (m[g.start:g.end] == GB.PREFILL).all()
        assert g.payload.data_ptr() == g.ptr and g.payload.numel() == nbytes
        if nbytes % 4 == 0 and skew % 4 == 0:
            import torch

            v = g.view(torch.float32)
            assert v.data_ptr() == g.ptr and v.numel() == nbytes // 4
        g.check()


def test_an_input_must_keep_its_bytes():
    a = np.arange(H * W, dtype=np.float32).reshape(H, W)
    for fill in GB.FILLS:
        g = GB.guarded_input(a, fill=fill, skew=4, name="frames")
        assert np.array_equal(g.numpy(np.float32, (H, W)), a)
        g.check()
        g.raw.numpy()[g.start + 17] ^= 1
        with pytest.raises(AssertionError, match=r"frames.*an input was written, payload offsets 17 \.\. 17 "):
            g.check()
        g = GB.guarded_input(a, fill=fill, name="frames")
        g.raw.numpy()[g.end] ^= 0x10
        with pytest.raises(AssertionError, match=r"frames.*BEHIND the payload, offsets 0 \.\. 0 "):
            g.check()


def test_bands_checks_every_array_and_never_drops_a_skew_silently():
    b = GB.Bands(GB.FILLS[1], device="cpu", skew=2)
    x = b.out("x", 64, itemsize=4)
    y = b.inp("y", np.zeros(8, np.uint8))
    z = b.inp("z", np.zeros(3, np.float64), skew=8)
    assert x.skew == 4 and y.skew == 2 and z.skew == 8 and x.fill == y.fill == GB.FILLS[1], "one element where 2 bytes do not fit"
    with pytest.raises(AssertionError, match="does not fit"):
        b.inp("w", np.zeros(3, np.float32), skew=2)
    aligned = GB.Bands(GB.FILLS[0], device="cpu")
    assert aligned.out("x", 64, itemsize=4).skew == 0 and aligned.inp("y", np.zeros(3, np.float64)).skew == 0
    b.check()
    y.raw.numpy()[y.start - 1] ^= 1
    with pytest.raises(AssertionError, match=r"y \(call\).*AHEAD of the payload, offsets -1 \.\. -1 "):
        b.check("call")


# ---------------------------------------------------------------------------------------------------------------------
# the table against the header
# ---------------------------------------------------------------------------------------------------------------------
def test_the_parser_finds_writable_device_pointers_only():
    text = """
    /* int oflk_commented(float *d_no); */
    int oflk_a(const float *d_in, float *d_out, unsigned char *d_mask, int n, void *stream);
    int oflk_b(const void *d_frames, void *d_state,
               const double *d_map, int *  d_count);
    int oflk_c(float *host_out, const float *const *d_levels);
    """
    assert GB.writable_device_pointers(text) == [("oflk_a", "d_out"), ("oflk_a", "d_mask"), ("oflk_b", "d_state"),
                                                 ("oflk_b", "d_count")]


def test_every_writable_device_pointer_of_the_header_is_covered_or_exempt():
    pairs = GB.writable_device_pointers()
    assert len(pairs) > 100 and len(set(pairs)) == len(pairs)
    missing = [p for p in pairs if p not in GB.COVERAGE]
    assert not missing, f"place these in guard_bands.COVERAGE (covered by a test, or exempt with the reason): {missing}"
    stale = [p for p in GB.COVERAGE if p not in set(pairs)]
    assert not stale, f"no such writable device pointer in include/oflk.h: {stale}"
    tests = set(re.findall(r"^def (test_\w+)\(", (GB.HEADER.parents[1] / GB.GPU_FILE).read_text(), flags=re.M))
    for pair, (kind, text) in GB.COVERAGE.items():
        assert kind in ("covered", "exempt"), pair
        if kind == "covered":
            assert text in tests, f"{pair}: {GB.GPU_FILE} has no {text}"
        else:
            assert len(text) > 20 and "\n" not in text, f"{pair}: an exemption gives its reason in one line"
