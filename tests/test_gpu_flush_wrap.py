"""oflk_stabilizer_flush_device where the frames that are left wrap the delay line: they lie in r + 1 slots, frame t in slot
t % (r + 1), so a flush of frames first .. first + count - 1 with first % (r + 1) + count > r + 1 takes two launches, and the
second one's output begins n0 frames of the layout (and n0 planes of `inside`) behind the first's.  That offset is the one
place of the flush where the bytes of a frame of the layout count, so every layout is run: float32, uint8, packed C = 3, NV12.

r = 3 and six pushes of 24 x 32 frames: first = 3, count = 3, slot 3 and then slots 0 and 1.  The reference is the host flush
of a stabiliser fed the same frames, which warps frame by frame from slot(t) and never forms that offset."""
import numpy as np
import pytest

import colour_model as CM
import motion_model as MM
import nv12_model as NM
import stabilize_model as SM

pytestmark = pytest.mark.gpu

R, PUSHES, H, W = 3, 6, 24, 32


def _frames(layout):
    grey, _ = SM.jitter_scene(5, T=PUSHES, H=H, W=W)
    if layout == "f32":
        return grey.astype(np.float32), {}
    if layout == "u8":
        return grey, {}
    if layout == "packed3":
        return CM.coloured(grey, 3), dict(channels=3)
    return NM.from_grey(grey), dict(nv12=True)


@pytest.mark.parametrize("layout", ["f32", "u8", "packed3", "nv12"])
def test_a_flush_that_wraps_the_delay_line_equals_the_host_flush(layout):
    import torch

    import _oflk

    frames, kw = _frames(layout)
    make = lambda: _oflk.Stabilizer(0, H, W, frames.dtype == np.uint8, 16, 4, MM.SIMILARITY, SM.weights(R), 32, 1.0, 2, 2, 5, 3,
                                    quality_level=0.05, min_distance=3.0, **kw)
    host, dev = make(), make()
    try:
        for f in frames:
            host.push(np.ascontiguousarray(f), True)
        first, want, _, want_in = host.flush(True)
        assert first == PUSHES - R and len(want) == R
        assert first % (R + 1) + R > R + 1, "the frames that are left wrap the delay line"
        d_frames = torch.from_numpy(frames).to("cuda:0")
        d_one = torch.empty_like(d_frames[0])
        d_out = torch.full((R,) + frames.shape[1:], 77, dtype=d_frames.dtype, device="cuda:0")
        d_ins = torch.full((R, H, W), 9, dtype=torch.uint8, device="cuda:0")
        for t in range(PUSHES):
            assert dev.push_device(d_frames[t].data_ptr(), d_one.data_ptr()) == (t - R if t >= R else -1)
        assert dev.flush_device(d_out.data_ptr(), d_ins.data_ptr()) == (first, R)
        torch.cuda.synchronize()
        SM.same(d_out.cpu().numpy(), want, f"{layout}: the flushed frames")
        SM.same(d_ins.cpu().numpy(), want_in, f"{layout}: inside")
    finally:
        host.close()
        dev.close()
