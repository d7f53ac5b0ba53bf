"""Guard bands: buffers that show a write outside them (used by tests/test_guard_bands_cpu.py, which needs no GPU:
python -m pytest tests/test_guard_bands_cpu.py -q, and by tests/test_gpu_guard_bands.py on an MI355X).

A kernel that stores a few bytes past the end of its output is invisible to a test that compares tensors of exactly the
output's size: the bytes land in whatever the allocator placed next, which is usually free.  `guarded` therefore lays an
array out as

    front band | payload | back band

in ONE allocation.  The payload starts `skew` bytes past a multiple of `align` (256 by default: the base decides between a
kernel's vector and element-wise instantiation) and its last byte is followed immediately by the back band, no rounding
slack.  A band is at least 4096 bytes and at least one full store tile of rows of the array it guards (`band_bytes`), so a
lane that misses its `y < H` check lands inside it.  The bands hold a byte pattern that depends on the position, never a
constant, and every guarded call runs under two fills that differ in every byte (`FILLS`): a stray byte can then equal the
pattern in at most one of the two runs.  `check` compares every byte of both bands, and for an input also every byte of
the payload.

COVERAGE (below) places every writable device pointer of include/oflk.h: covered by a test of
tests/test_gpu_guard_bands.py, or exempt with the reason.  tests/test_guard_bands_cpu.py holds the table to the header.
"""
import re
from pathlib import Path

import numpy as np

MIN_BAND = 4096
TILE_ROWS = 16      # the tallest store tile of the library: kPTH = kUTH = kCsTH = 16
FILLS = (0x3C, 0x3C ^ 0xFF)
PREFILL = 0x77      # every payload byte of an output before the call (float32 5.0e33, int32 2004318071)


def band_bytes(nbytes, row_bytes=None):
    """bytes of one band: 4096 at least, and TILE_ROWS rows of the array (the whole array again where it is smaller)"""
    rows = nbytes if row_bytes is None else min(TILE_ROWS * int(row_bytes), nbytes)
    return max(MIN_BAND, int(rows))


def pattern(offsets, fill):
    """the band byte at `offsets` (int64, relative to the payload's start: negative in the front band, >= nbytes behind)"""
    o = np.asarray(offsets, np.int64)
    return (((o * 37) ^ (o >> 8) * 11 ^ (o >> 16)) & 0xFF).astype(np.uint8) ^ np.uint8(fill)


class Guarded:
    """one allocation: front band, payload, back band.  Offsets in messages are relative to the payload: the front band
    counts from the payload's start (-1 is the byte ahead of it), the back band from its end (0 is the byte behind it)."""

    def __init__(self, nbytes, *, align=256, skew=0, fill=FILLS[0], device="cpu", row_bytes=None, name="buffer", data=None):
        import torch

        nbytes = int(nbytes)
        assert nbytes >= 0 and align >= 1 and 0 <= skew < align and 0 <= fill <= 0xFF
        self.name, self.nbytes, self.align, self.skew, self.fill = name, nbytes, int(align), int(skew), int(fill)
        self.band = band_bytes(nbytes, row_bytes)
        self.raw = torch.empty(self.band + align + nbytes + self.band, dtype=torch.uint8, device=device)
        a0 = self.raw.data_ptr()
        self.start = self.band + (skew - (a0 + self.band)) % align      # offset of the payload in the allocation
        self.end = self.start + nbytes
        self.front, self.back = self.start, self.band                    # band sizes; the front one takes the slack
        self.ptr = a0 + self.start
        assert (self.ptr - skew) % align == 0 and self.end + self.back <= self.raw.numel()
        self.raw = self.raw[:self.end + self.back]
        self.input = None
        self._want_front = torch.from_numpy(pattern(np.arange(-self.front, 0), fill)).to(device)
        self._want_back = torch.from_numpy(pattern(np.arange(nbytes, nbytes + self.back), fill)).to(device)
        self.raw[:self.start] = self._want_front
        self.raw[self.end:] = self._want_back
        if data is None:
            self.raw[self.start:self.end] = PREFILL
        else:
            b = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
            assert b.size == nbytes, f"{name}: {b.size} bytes given for a payload of {nbytes}"
            self.input = torch.from_numpy(b.copy()).to(device)
            self.raw[self.start:self.end] = self.input

    @property
    def payload(self):
        """the payload's bytes, a view"""
        return self.raw[self.start:self.end]

    def view(self, dtype):
        """a typed view of the payload (torch dtype); the skew must be a multiple of the element size"""
        return self.payload.view(dtype)

    def numpy(self, dtype=np.uint8, shape=None):
        """a host copy of the payload as `dtype` (any skew)"""
        a = self.payload.cpu().numpy().copy().view(dtype)
        return a if shape is None else a.reshape(shape)

    def band_byte(self, side, offset):
        """the pattern's byte at `offset` of a band, in the offsets of the messages"""
        return int(pattern([offset if side == "front" else self.nbytes + offset], self.fill)[0])

    def _dirty(self, got, want):
        import torch

        bad = torch.nonzero(got != want).reshape(-1)
        return None if bad.numel() == 0 else (int(bad[0]), int(bad[-1]), int(bad.numel()))

    def check(self, what=""):
        """every byte of both bands; of an input every payload byte too"""
        where = f"{self.name}{' (' + what + ')' if what else ''}, fill 0x{self.fill:02X}, skew {self.skew}"
        d = self._dirty(self.raw[:self.start], self._want_front)
        if d:
            raise AssertionError(f"{where}: written AHEAD of the payload, offsets {d[0] - self.front} .. {d[1] - self.front} "
                                 f"from its start ({d[2]} bytes)")
        d = self._dirty(self.raw[self.end:], self._want_back)
        if d:
            raise AssertionError(f"{where}: written BEHIND the payload, offsets {d[0]} .. {d[1]} from its end ({d[2]} bytes)")
        if self.input is not None:
            d = self._dirty(self.payload, self.input)
            if d:
                raise AssertionError(f"{where}: an input was written, payload offsets {d[0]} .. {d[1]} ({d[2]} bytes)")


def guarded(nbytes, *, align=256, skew=0, fill=FILLS[0], device="cpu", row_bytes=None, name="buffer"):
    """an output, a workspace or a state of `nbytes`, prefilled with PREFILL"""
    return Guarded(nbytes, align=align, skew=skew, fill=fill, device=device, row_bytes=row_bytes, name=name)


def guarded_input(array, *, align=256, skew=0, fill=FILLS[0], device="cpu", row_bytes=None, name="input"):
    """an input: the array's bytes as the payload; `check` then also asserts that they are unchanged"""
    a = np.ascontiguousarray(array)
    return Guarded(a.nbytes, align=align, skew=skew, fill=fill, device=device, row_bytes=row_bytes, name=name, data=a)


class Bands:
    """the guarded arrays of one call: `out` / `inp` make them, `check` asserts them all.  `skew` is the run's: 0 puts
    every array on its 256-byte boundary, anything else skews every array (see _skew)"""

    def __init__(self, fill, device="cuda:0", skew=0):
        self.fill, self.device, self.skew, self.all = fill, device, skew, []

    def _skew(self, itemsize, skew):
        """a skew given for this array must fit its elements; the run's skew is taken where it fits them, and is one element
        of the array where it does not (a float32 array in a run skewed by 1 or 2 bytes lies 4 bytes off): never silently 0"""
        if skew is not None:
            assert skew % itemsize == 0, f"a skew of {skew} bytes does not fit elements of {itemsize}"
            return skew
        return self.skew if self.skew % itemsize == 0 else itemsize

    def out(self, name, nbytes, row_bytes=None, itemsize=1, skew=None):
        g = guarded(nbytes, skew=self._skew(itemsize, skew), fill=self.fill, device=self.device, row_bytes=row_bytes, name=name)
        self.all.append(g)
        return g

    def inout(self, name, array, row_bytes=None, skew=None):
        """an array the call reads and writes: loaded with `array`, bands checked, the payload left to the caller"""
        g = self.inp(name, array, row_bytes, skew)
        g.input = None
        return g

    def inp(self, name, array, row_bytes=None, skew=None):
        a = np.ascontiguousarray(array)
        g = guarded_input(a, skew=self._skew(a.itemsize, skew), fill=self.fill, device=self.device, row_bytes=row_bytes,
                          name=name)
        self.all.append(g)
        return g

    def check(self, what=""):
        for g in self.all:
            g.check(what)


# ---------------------------------------------------------------------------------------------------------------------
# the header: every writable device pointer
# ---------------------------------------------------------------------------------------------------------------------
HEADER = Path(__file__).resolve().parents[1] / "include" / "oflk.h"
GPU_FILE = "tests/test_gpu_guard_bands.py"


def writable_device_pointers(text=None):
    """[(function, parameter)] of every prototype parameter that is a pointer to non-const named d_*"""
    src = HEADER.read_text() if text is None else text
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^\s*#.*$", " ", src, flags=re.M)
    pairs = []
    for m in re.finditer(r"\b(\w+)\s*\(([^()]*)\)\s*;", src):
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            q = re.match(r"^(.*\*)\s*(d_\w+)$", p)
            if q and not re.match(r"^const\b", q.group(1)):
                pairs.append((m.group(1), q.group(2)))
    return pairs


def _cover(test, fn, *params):
    return {(fn, p): ("covered", test) for p in params}


def _exempt(reason, fn, *params):
    return {(fn, p): ("exempt", reason) for p in params}


COVERAGE = {}
for _fn in ("oflk_warp_affine", "oflk_warp_perspective"):
    COVERAGE.update(_cover("test_warp_planar", _fn, "d_out", "d_inside"))
for _fn in ("oflk_warp_affine_packed", "oflk_warp_perspective_packed"):
    COVERAGE.update(_cover("test_warp_packed", _fn, "d_out", "d_inside"))
for _fn in ("oflk_warp_affine_nv12", "oflk_warp_perspective_nv12"):
    COVERAGE.update(_cover("test_warp_nv12", _fn, "d_out", "d_inside"))
COVERAGE.update(_cover("test_luma", "oflk_luma_u8", "d_luma"))
COVERAGE.update(_cover("test_fb_consistency", "oflk_fb_consistency", "d_err_f", "d_err_b", "d_valid_f", "d_valid_b"))
COVERAGE.update(_cover("test_flow_median", "oflk_flow_median", "d_out"))
COVERAGE.update(_cover("test_interpolate_planar", "oflk_interpolate_frames", "d_out", "d_status"))
COVERAGE.update(_cover("test_interpolate_packed", "oflk_interpolate_frames_packed", "d_out", "d_status"))
COVERAGE.update(_cover("test_interpolate_nv12", "oflk_interpolate_frames_nv12", "d_out", "d_status"))
COVERAGE.update(_cover("test_stabilize_trajectory", "oflk_stabilize_trajectory", "d_correction", "d_map", "d_held"))
COVERAGE.update(_cover("test_stabilize_trajectory_ring", "oflk_stabilize_trajectory_ring", "d_correction", "d_map"))
COVERAGE.update(_cover("test_mosaic_chain", "oflk_mosaic_chain", "d_from_anchor", "d_to_anchor", "d_box", "d_held", "d_dropped"))
for _fn in ("oflk_mosaic_accumulate", "oflk_mosaic_accumulate_exposure"):
    COVERAGE.update(_cover("test_mosaic_accumulate_and_resolve", _fn, "d_state"))
COVERAGE.update(_cover("test_mosaic_accumulate_and_resolve", "oflk_mosaic_resolve", "d_out", "d_count"))
COVERAGE.update(_cover("test_mosaic_median", "oflk_mosaic_median", "d_out", "d_count"))
for _fn in ("oflk_plan_single_scale", "oflk_plan_single_scale_u8", "oflk_plan_single_scale_fp16"):
    COVERAGE.update(_cover("test_dense_single_scale", _fn, "d_u", "d_v"))
for _fn in ("oflk_plan_pyramidal", "oflk_plan_pyramidal_u8", "oflk_plan_pyramidal_sequence", "oflk_plan_pyramidal_sequence_u8"):
    COVERAGE.update(_cover("test_dense_pyramidal", _fn, "d_u", "d_v"))
for _fn in ("oflk_plan_pyramidal_sequence_fb", "oflk_plan_pyramidal_sequence_fb_u8"):
    COVERAGE.update(_cover("test_dense_pyramidal", _fn, "d_uf", "d_vf", "d_ub", "d_vb"))
for _fn in ("oflk_plan_resolve_uncertain", "oflk_plan_resolve_uncertain_u8"):     # on pairs flagged by construction
    COVERAGE.update(_cover("test_dense_resolve_uncertain", _fn, "d_u", "d_v"))
for _fn in ("oflk_plan_resolve_uncertain_sequence_fb", "oflk_plan_resolve_uncertain_sequence_fb_u8"):
    COVERAGE.update(_cover("test_dense_resolve_uncertain", _fn, "d_uf", "d_vf", "d_ub", "d_vb"))
COVERAGE.update(_cover("test_track_points", "oflk_track_points", "d_tracks", "d_visible"))
COVERAGE.update(_cover("test_sparse_tracks", "oflk_plan_sparse_tracks", "d_tracks", "d_visible"))
COVERAGE.update(_cover("test_sparse_klt_replenish", "oflk_plan_sparse_klt_replenish", "d_workspace", "d_qt", "d_qxy", "d_tracks",
                       "d_visible", "d_born", "d_detected", "d_residual"))
COVERAGE.update(_cover("test_corner_score", "oflk_corner_score", "d_score"))
COVERAGE.update(_cover("test_good_features", "oflk_good_features", "d_workspace", "d_count", "d_xy", "d_score"))
COVERAGE.update(_cover("test_replenish_features", "oflk_replenish_features", "d_workspace", "d_qt", "d_qxy", "d_born", "d_detected"))
for _fn in ("oflk_estimate_motion", "oflk_tracks_motion", "oflk_estimate_homography", "oflk_tracks_homography"):
    COVERAGE.update(_cover("test_fits", _fn, "d_workspace", "d_model", "d_inlier", "d_counts"))
for _fn in ("oflk_align_refine", "oflk_align_sequence"):
    COVERAGE.update(_cover("test_align", _fn, "d_workspace", "d_model_out", "d_status_out", "d_stats"))
for _fn in ("oflk_align_refine_photo", "oflk_align_sequence_photo", "oflk_align_refine_robust", "oflk_align_sequence_robust"):
    COVERAGE.update(_cover("test_align", _fn, "d_workspace", "d_model_out", "d_status_out", "d_stats", "d_photo_out"))
COVERAGE.update(_cover("test_align_weights", "oflk_align_weights", "d_weights"))
COVERAGE.update(_cover("test_u8_to_f32", "oflk_u8_to_f32", "d_out"))
COVERAGE.update(_cover("test_rtl_flow_device", "oflk_rtl_flow_u8_device", "d_u", "d_v"))
for _fn in ("oflk_stabilizer_push_device", "oflk_stabilizer_flush_device"):
    COVERAGE.update(_cover("test_stabilizer_push_and_flush_device", _fn, "d_out", "d_inside"))
