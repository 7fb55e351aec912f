"""``ysmr_thrview_batch`` on the device against its host twin ``ysmr_thrview_batch_host`` (which tests/test_thrview_cpu.py
holds to tests/thrview_model.py) on the shapes of the model: every output byte equal, 64 guard bytes on either side of the
output and the gaps between frames untouched, the padding of every stored row zero."""
import numpy as np
import pytest

import thrview_model as T
from test_thrview_cpu import FILL, GAP, case, host

pytestmark = pytest.mark.gpu

GUARD = 64


def launch(frames, cls, mask, mode, bottom_up, stride, frame_bytes):
    """-> (the n * frame_bytes output bytes, the guard bytes in front, the guard bytes behind)."""
    import torch
    from ysmr_amd import _lib
    n, h, w = cls.shape
    channels = 1 if frames.ndim == 3 else 3
    dev = torch.device("cuda:0")
    on_dev = [torch.from_numpy(np.array(a)).to(dev) for a in (frames, cls, mask)]
    block = torch.full((GUARD + n * frame_bytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
    # (pointers the mode does not read are NULL, as the pipeline's call has them)
    rc = _lib.lib().ysmr_thrview_batch(_lib.stream_ptr(dev), on_dev[0].data_ptr() if mode == T.CLASSES else None, on_dev[1].data_ptr(),
                                       None if mode == T.MARKERS else on_dev[2].data_ptr(), n, h, w, channels, mode,
                                       block.data_ptr() + GUARD, stride, frame_bytes, bottom_up)
    _lib.check(rc, "ysmr_thrview_batch")
    torch.cuda.synchronize(dev)
    got = block.cpu().numpy()
    return got[GUARD:-GUARD].reshape(n, frame_bytes), got[:GUARD], got[-GUARD:]


@pytest.mark.parametrize("mode", sorted(T.MODES))
@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_kernel_stores_what_the_host_twin_stores(shape, mode):
    n, h, w = shape
    code = T.MODES[mode]
    tight = (3 * w + 3) & ~3
    for channels in (1, 3):
        frames, cls, mask = case(shape, channels)
        for bottom_up in (0, 1):
            for stride, gap in ((tight, 0), (tight + 8, GAP)):
                frame_bytes = stride * h + gap
                got, front, behind = launch(frames, cls, mask, code, bottom_up, stride, frame_bytes)
                want = host(frames, cls, mask, code, bottom_up, stride, frame_bytes)
                what = "channels {}, bottom_up {}, stride {}".format(channels, bottom_up, stride)
                assert np.array_equal(got, want), "{}: {} bytes differ".format(what, int((got != want).sum()))
                assert (front == FILL).all() and (behind == FILL).all(), what
                assert (got[:, stride * h:] == FILL).all(), what                          # the bytes between two frames are the caller's
                assert (got[:, :stride * h].reshape(n, h, stride)[:, :, 3 * w:] == 0).all(), what


def test_refused_arguments_launch_nothing_and_write_nothing():
    import torch
    from ysmr_amd import _lib
    frames, cls, mask = case((3, 3, 5), 1)
    dev = torch.device("cuda:0")
    f, c, m = (torch.from_numpy(np.array(a)).to(dev) for a in (frames, cls, mask))
    out = torch.full((3, 48), FILL, dtype=torch.uint8, device=dev)
    L = _lib.lib()

    def call(**kw):
        a = dict(frames=f.data_ptr(), cls=c.data_ptr(), mask=m.data_ptr(), channels=1, mode=2, out=out.data_ptr(), stride=16, fb=48)
        a.update(kw)
        return L.ysmr_thrview_batch(_lib.stream_ptr(dev), a["frames"], a["cls"], a["mask"], 3, 3, 5, a["channels"], a["mode"], a["out"],
                                    a["stride"], a["fb"], 0)

    for what, kw in {"cls": dict(cls=None), "out": dict(out=None), "mask, mode 0": dict(mask=None, mode=0), "mask, mode 2": dict(mask=None),
                     "frames": dict(frames=None), "channels": dict(channels=2), "mode": dict(mode=3), "stride": dict(stride=12),
                     "frame bytes": dict(fb=44), "alignment": dict(out=out.data_ptr() + 2)}.items():
        assert call(**kw) == _lib.YSMR_ERR_ARG, what
        assert L.ysmr_last_error().decode().startswith("thrview: "), what
    torch.cuda.synchronize(dev)
    assert (out.cpu().numpy() == FILL).all()
    assert call() == _lib.YSMR_OK
    torch.cuda.synchronize(dev)
    assert np.array_equal(out.cpu().numpy(), host(frames, cls, mask, T.CLASSES, 0, 16, 48))


def test_two_runs_give_the_same_bytes():
    frames, cls, mask = case((2, 3, 1040), 3)
    stride = 3 * 1040
    a = launch(frames, cls, mask, T.CLASSES, 1, stride, stride * 3)[0]
    b = launch(frames, cls, mask, T.CLASSES, 1, stride, stride * 3)[0]
    assert np.array_equal(a, b)
