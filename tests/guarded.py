"""Device buffers with guard bytes, for the tests that hold an entry point of include/pasnl.h to the sizes the header states
(tests/test_gpu_grad_edges.py: the backward; tests/test_gpu_abi_bounds.py: the forward entries and their workspaces).

A `Guarded` view is `nbytes` bytes in the middle of one larger allocation that is pre-filled with one byte value.  Everything a
kernel could reach by running a row or a tile past the end of the view is memory this buffer owns: a stray store is a changed
guard byte and a failed assertion, never a fault."""
import numpy as np
import torch

GUARD = 256  # bytes on either side of a view (keeps the view's alignment)

NAN_BYTE = 0xFF   # four of them are a NaN, and -1 as an int32
WS_BYTE = 0xA5
# the second run of tests/test_gpu_abi_bounds.py: other bytes in the outputs, zeros in the workspace
ALT_BYTE = 0x5A
ALT_WS_BYTE = 0x00


def output_guard(row_bytes):
    """guard of an output: the larger of 4 KiB and one output row, rounded up to 256 bytes (catches a stray whole row)"""
    return (max(4096, int(row_bytes)) + 255) // 256 * 256


class Guarded:
    """`nbytes` bytes inside a larger device buffer that is pre-filled with one byte value"""

    def __init__(self, nbytes, fill, guard=GUARD):
        assert guard % 256 == 0
        self.nbytes, self.fill, self.guard = nbytes, fill, guard
        self.buf = torch.full((guard + nbytes + guard,), fill, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + guard

    def inside(self):
        return self.buf[self.guard:self.guard + self.nbytes]

    def floats(self, shape):
        return self.inside().view(torch.float32).reshape(shape).cpu().numpy()

    def array(self, shape, dtype):
        """the view's bytes as a numpy array of `dtype` (any itemsize) and `shape`"""
        return self.inside().cpu().numpy().view(np.dtype(dtype)).reshape(shape)

    def guards_intact(self):
        return bool((self.buf[:self.guard] == self.fill).all()) and bool((self.buf[self.guard + self.nbytes:] == self.fill).all())

    def untouched(self):
        return self.guards_intact() and bool((self.inside() == self.fill).all())
