"""Guarded device buffers for the kernel tests (tests/test_gpu_fedopt_kernels.py,
tests/test_gpu_fedavg_kernels.py): P elements between two runs of 64 sentinel elements, a NaN pattern no
computation in those tests produces, so that a store outside the buffer and an element never stored both
show."""
import numpy as np
import torch

DEV = "cuda:0"
GUARD = 64
TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64,
            "i32": torch.int32, "i64": torch.int64}
_INT_VIEW = {2: torch.int16, 4: torch.int32, 8: torch.int64}
_NP_INT = {2: np.int16, 4: np.int32, 8: np.int64}
SENTINEL = {2: 0x7DAD, 4: 0x7FA5A5A5, 8: 0x7FF5A5A5A5A5A5A5}      # NaNs no computation here produces


class Buf:
    """P elements at a 16-B aligned address (+ ``shift`` elements), 64 sentinel elements on each side."""

    def __init__(self, P, name, shift=0, data=None):
        tdt = TORCH_DT[name]
        self.P, self.lo = P, GUARD + shift
        self.full = torch.empty(GUARD + shift + P + GUARD, dtype=tdt, device=DEV)
        self.size = self.full.element_size()
        self.full.view(_INT_VIEW[self.size]).fill_(SENTINEL[self.size])
        self.t = self.full[self.lo:self.lo + P]
        assert self.t.data_ptr() % 16 == (shift * self.size) % 16
        self.bits0 = None
        if data is not None:
            data = np.ascontiguousarray(data)
            if name == "bf16":            # an f32 array with zero low halves: the bf16 bits are the high ones,
                w = data.view(np.uint32)  # uploaded as they are (NaN payloads included)
                assert data.dtype == np.float32 and not (w & 0xFFFF).any()
                self.bits0 = (w >> 16).astype(np.uint16).view(np.int16)
                self.t.view(torch.int16).copy_(torch.from_numpy(self.bits0))
            else:
                self.bits0 = data.view(_NP_INT[self.size])
                self.t.copy_(torch.from_numpy(data))

    def bits(self):
        """The P elements as integers of their size (host)."""
        return self.t.view(_INT_VIEW[self.size]).cpu().numpy()

    def check(self, what, written):
        bits = self.full.view(_INT_VIEW[self.size]).cpu().numpy()
        s = _NP_INT[self.size](SENTINEL[self.size])
        assert (bits[:self.lo] == s).all() and (bits[self.lo + self.P:] == s).all(), f"{what}: a guard was written"
        if written:
            left = int((bits[self.lo:self.lo + self.P] == s).sum())
            assert left == 0, f"{what}: {left} of {self.P} elements were not written"

    def check_unchanged(self, what):
        """An input buffer: its guards and every bit of the data it was created with."""
        self.check(what, False)
        assert self.bits0 is not None and np.array_equal(self.bits(), self.bits0), f"{what}: an input was overwritten"

    def numpy(self):
        return self.t.cpu().numpy()
