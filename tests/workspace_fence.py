"""A device workspace of exactly the size its jpegx_*_workspace_bytes* function declares, at the weakest alignment the
entry accepts, between two guards: what an integrator gets who sub-allocates workspaces from an arena.
The conventions are those of fenced.py (0xA5, the messages); a plain helper module of the suite.

An entry has no size argument to check, so "the size function's value is enough" is its whole contract.  hipMalloc's
granularity and the shared 64..96 MiB buffers of the road modules hide an overrun of any length; here an overrun of up to
a whole span (64 KiB at least: table-sized strides) lands in the guard behind, and every run starts from a workspace that
holds the canary in every byte: a word that a call reads before it has written it is 0xA5A5A5A5, never a zero."""
import re

import numpy as np

from fenced import CANARY

FRONT = 4096                 # bytes in front of the span at least
BEHIND = 64 << 10            # bytes behind the span at least; the guard is as long as the span where that is more

# size function -> ids of the tests that run an entry on its fenced workspace; filled when the modules below are imported
REGISTRY = {}
MODULES = ["test_gpu_workspace_entropy", "test_gpu_workspace_batch_8", "test_gpu_workspace_batch_n", "test_gpu_workspace_sets",
           "test_gpu_workspace_probes"]


def fences(*names):
    """Decorator of a GPU test: it runs every entry that carves the workspace of the size functions `names`."""
    def mark(fn):
        for name in names:
            REGISTRY.setdefault(name, []).append("%s::%s" % (fn.__module__, fn.__name__))
        return fn
    return mark


def declared(header_text):
    """The exported size functions of include/jpegx.h: every declared name that matches *_workspace_bytes*."""
    return sorted(set(re.findall(r"^size_t\s+(jpegx_\w*_workspace_bytes\w*)\s*\(", header_text, re.M)))


class FencedWorkspace:
    """One device allocation: guard, span of exactly `nbytes`, guard -- every byte 0xA5.  `ptr`, the span's first byte, is
    a multiple of `align` and NOT of 2 * align."""

    def __init__(self, gpu, nbytes, align=16):
        assert nbytes > 0 and align >= 16 and align & (align - 1) == 0, (nbytes, align)
        self.gpu, self.nbytes, self.align = gpu, int(nbytes), int(align)
        self.behind = max(BEHIND, self.nbytes)
        self.buf = gpu.DeviceBuffer(FRONT + 2 * self.align + self.nbytes + self.behind)
        self.at = FRONT + (self.align - (self.buf.ptr + FRONT)) % (2 * self.align)
        self.ptr = self.buf.ptr + self.at
        assert self.ptr % self.align == 0 and self.ptr % (2 * self.align) != 0
        assert self.at >= FRONT and self.at + self.nbytes + self.behind <= self.buf.nbytes
        self.fill()

    def fill(self):
        """The whole allocation, span included, back to the canary."""
        self.gpu.check(self.gpu.lib().jpegx_memset(self.buf.ptr, CANARY, self.buf.nbytes, None), "jpegx_memset")
        self.gpu.check(self.gpu.lib().jpegx_device_synchronize())

    def check(self, what):
        """After a device-wide synchronise: both guards hold the canary still."""
        self.gpu.check(self.gpu.lib().jpegx_device_synchronize())
        raw = self.buf.download((self.buf.nbytes,), np.uint8)
        end = self.at + self.nbytes
        bad = np.flatnonzero(raw[end:] != CANARY)
        assert bad.size == 0, ("%s: %d bytes behind the workspace's %d bytes were written, the first %d bytes behind its end"
                               % (what, bad.size, self.nbytes, bad[0]))
        bad = np.flatnonzero(raw[:self.at] != CANARY)
        assert bad.size == 0, ("%s: %d bytes in front of the workspace were written, the first %d bytes in front of its base, "
                               "%d in front of its end" % (what, bad.size, self.at - bad[0], end - bad[0]))

    def free(self):
        self.buf.free()
