"""Shared by the GPU test files that call kernels directly: sentinel-guarded, NaN-filled output buffers (Guard) and NaN-poisoning of the allocator blocks a
node is about to receive (_poison).  An unwritten row or tail pixel then shows as NaN instead of as the previous test's correct value, and a store one past
the end shows as a broken sentinel without any fault."""
import math

import torch

NAN = float('nan')


def _poison(*like):
    """fill allocator blocks of the sizes about to be handed out with NaN, then free them: an element a kernel leaves unwritten is then NaN, not the
    previous test's correct value"""
    for t in like:
        if t is not None and t.is_floating_point():
            p = torch.full_like(t, NAN)
            del p


class Guard:
    """outputs of direct C-ABI calls: each inside a larger buffer with 256 sentinel elements on both sides and NaN in the body"""
    SENT = 7.0

    def __init__(self):
        self.items = []

    def new(self, shape, dtype, what):
        n = math.prod(shape)
        buf = torch.full((n + 512,), self.SENT, dtype=dtype, device='cuda')
        body = buf[256:256 + n]
        if dtype.is_floating_point:
            body.fill_(NAN)
        else:
            body.fill_(85)
        self.items.append((buf, n, what))
        return body.view(shape)

    def check(self, nan_ok=()):
        for buf, n, what in self.items:
            b = buf.cpu()
            assert bool((b[:256] == self.SENT).all()) and bool((b[256 + n:] == self.SENT).all()), f'{what}: a sentinel next to the output was overwritten'
            if b.dtype.is_floating_point and what not in nan_ok:
                assert not bool(torch.isnan(b[256:256 + n]).any()), f'{what}: {int(torch.isnan(b[256:256 + n]).sum())} elements were never written'
