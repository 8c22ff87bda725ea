"""What the GPU tests share: uploads, guard bands, the byte compare of record arrays and the models with
their fitter.  torch is imported where it is used, so collecting the tests needs no GPU."""
import contextlib

import numpy as np

GUARD, FILL = 4096, 0xA5


def to_device(array):
    """The bytes of `array` on the device, as a flat uint8 tensor."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).cuda()


def guarded(nbytes, skew=0):
    """A device buffer of 4 KB guard bands around `nbytes` at a skewed start: (tensor, pointer, offset)."""
    import torch
    buf = torch.full((GUARD + skew + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + GUARD + skew, GUARD + skew


def untouched(buf, off, nbytes):
    """Whether everything of `buf` (a device tensor or a host array of bytes) outside [off, off + nbytes) still holds the fill."""
    host = buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()
    return bool((host[:off] == FILL).all() and (host[off + nbytes:] == FILL).all())


def between_guards(frames, guard, fill):
    """The frames on the device inside a larger allocation, `guard` elements of depth `fill` before and after: (the tensor of the
    frames' shape, the allocation, which must stay alive)."""
    import torch
    flat = np.full(frames.size + 2 * guard, fill, np.uint16)
    flat[guard:guard + frames.size] = frames.reshape(-1)
    whole = torch.from_numpy(flat.view(np.int16)).cuda()
    return whole[guard:guard + frames.size].view(*frames.shape), whole


def same_records(got, want, what):
    """Two record arrays byte for byte: length, item size, every record (so that a failure names the record), the whole buffer."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert len(got) == len(want), (what, len(got), len(want))
    assert got.dtype.itemsize == want.dtype.itemsize, (what, got.dtype.itemsize, want.dtype.itemsize)
    for i in range(len(want)):
        assert got[i].tobytes() == want[i].tobytes(), (what, i, got[i], want[i])
    assert got.tobytes() == want.tobytes(), what


@contextlib.contextmanager
def fit_models(host_models):
    """(models, fitter) for a list or a dict of (pts, nrm, ...): fit.Model of each and one fit.Fitter; the fitter is closed first."""
    from depthhead_amd import fit
    if isinstance(host_models, dict):
        ms = {k: fit.Model(m[0], m[1]) for k, m in host_models.items()}
    else:
        ms = [fit.Model(m[0], m[1]) for m in host_models]
    ft = fit.Fitter()
    try:
        yield ms, ft
    finally:
        ft.close()
        for m in (ms.values() if isinstance(ms, dict) else ms):
            m.close()
