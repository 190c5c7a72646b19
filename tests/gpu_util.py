"""Helpers for the -m gpu parity tests: torch is only device memory here."""
import numpy as np
import torch


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def ptr(t):
    return t.data_ptr()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# a quiet NaN whose payload no kernel produces: padding words that must be neither read (a read turns results into
# NaN) nor written (the bits change)
CANARY = 0x7FF8DEADBEEF0001


class Canaried:
    """A rows x cols float64 array with row stride `ld` inside a larger device buffer: the base is `off` elements into a
    16-byte aligned allocation (off = 1: an 8-byte aligned base), and every word outside the rows x cols window --
    padding columns, the words before the base, a tail of `tail` words after the last row -- holds CANARY."""

    def __init__(self, a, ld=None, off=0, tail=256):
        a = np.asarray(a, dtype=np.float64)
        self.vector = a.ndim == 1
        a2 = a.reshape(1, -1) if self.vector else a
        self.shape = a2.shape
        self.ld = self.shape[1] if ld is None else ld
        assert self.ld >= self.shape[1]
        self.off = off
        self.buf = torch.full((off + self.shape[0] * self.ld + tail,), CANARY, dtype=torch.int64, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.set(a)

    def window(self):
        r, c = self.shape
        return self.buf.view(torch.float64)[self.off:self.off + r * self.ld].view(r, self.ld)[:, :c]

    def set(self, a):
        self.window().copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(self.shape)))

    @property
    def ptr(self):
        return self.buf.data_ptr() + 8 * self.off

    def get(self):
        w = self.window().cpu().numpy()
        return w[0].copy() if self.vector else w.copy()

    def padding_intact(self):
        h = self.buf.cpu().numpy()
        mask = np.ones(h.size, dtype=bool)
        r, c = self.shape
        idx = self.off + (np.arange(r)[:, None] * self.ld + np.arange(c)[None, :])
        mask[idx.ravel()] = False
        return bool((h[mask] == CANARY).all())
