"""Rectangle obstacles (dgppo/env/obstacle.py:30-105) as packed 16-float device records.

Record layout (include/dgppo_hip.h, DGPPO_OBST_FIELDS):
    [cx, cy, width, height, theta, cos(theta), sin(theta), type, p0x, p0y, p1x, p1y, p2x, p2y, p3x, p3y]
`Rectangle` exposes the reference's field names as views of that record (no copies); the reset kernels
create the rectangles on the GPU, `Rectangle.create` builds them on the host with the same arithmetic
(dgppo_make_rectangles) for scenes of the caller's own.
"""
from __future__ import annotations

import ctypes

import torch

OBST_FIELDS = 16


class Rectangle:
    __slots__ = ("packed",)

    def __init__(self, packed: torch.Tensor):
        assert packed.shape[-1] == OBST_FIELDS
        self.packed = packed

    @classmethod
    def create(cls, center, width, height, theta) -> "Rectangle":
        """Rectangle.create (dgppo/env/obstacle.py:39-56), batched: center (..., 2), width / height / theta (...)
        -> packed records (..., 16) on the tensors' device.  Computed on the host by dgppo_make_rectangles (the
        reset kernels' fp32 sin / cos and operation order), then copied to the device once."""
        from .. import _lib

        center = torch.as_tensor(center, dtype=torch.float32)
        if center.dim() < 1 or center.shape[-1] != 2:
            raise ValueError(f"Rectangle.create: center must be (..., 2), got {tuple(center.shape)}")
        dev, shape = center.device, tuple(center.shape[:-1])
        host = [center.detach().cpu().contiguous()]
        for name, t in (("width", width), ("height", height), ("theta", theta)):
            t = torch.as_tensor(t, dtype=torch.float32)
            if tuple(t.shape) != shape:
                raise ValueError(f"Rectangle.create: {name} must be {shape}, got {tuple(t.shape)}")
            host.append(t.detach().cpu().contiguous())
        out = torch.empty(shape + (OBST_FIELDS,), dtype=torch.float32)
        count = out.numel() // OBST_FIELDS
        _lib.check(_lib.load().dgppo_make_rectangles(count, *(ctypes.c_void_p(t.data_ptr()) for t in host),
                                                     ctypes.c_void_p(out.data_ptr())), "dgppo_make_rectangles")
        return cls(out.to(dev))

    @property
    def type(self):
        return self.packed[..., 7:8]

    @property
    def center(self):
        return self.packed[..., 0:2]

    @property
    def width(self):
        return self.packed[..., 2]

    @property
    def height(self):
        return self.packed[..., 3]

    @property
    def theta(self):
        return self.packed[..., 4]

    @property
    def points(self):
        return self.packed[..., 8:16].unflatten(-1, (4, 2))

    @property
    def n(self) -> int:
        return self.packed.shape[-2]

    def _map_tensors(self, fn):
        return Rectangle(fn(self.packed))

    def __getitem__(self, idx):
        return Rectangle(self.packed[idx])
