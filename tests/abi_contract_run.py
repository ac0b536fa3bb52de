"""Device-side plumbing shared by tests/test_gpu_abi_guard_bands.py and tests/test_gpu_abi_stream_order.py: puts the
arrays of a case of tests/abi_contract_cases.py into device memory the way the header allows a caller to, every
output and scratch buffer between two guard bands of a sentinel bit pattern."""
import ctypes

import numpy as np

GUARD = 4096          # bytes on either side, at least; at least one innermost row of the output
# a quiet NaN with a payload for the float types, 0x5A bytes for the integers: neither is a value any case expects
SENTINEL = {np.dtype(np.float32): np.array([0x7FE5A5A5], np.uint32).view(np.float32)[0],
            np.dtype(np.float64): np.array([0x7FF8A5A5A5A5A5A5], np.uint64).view(np.float64)[0]}


def sentinel_bytes(dtype):
    dtype = np.dtype(dtype)
    if dtype in SENTINEL:
        return np.frombuffer(SENTINEL[dtype].tobytes(), np.uint8)
    return np.full(dtype.itemsize, 0x5A, np.uint8)


class Region:
    """``nbytes`` of device memory for an array of ``dtype`` inside a sentinel-filled buffer.  The pointer has
    exactly the alignment asked for: ``align`` >= 16 as it is, a smaller one (the natural alignment of the type, where
    the header demands none) with the next power of two broken, ``align`` 0 at ``offset_elems`` elements off 16."""

    def __init__(self, gpu, nbytes, dtype, align, offset_elems=0, row_bytes=0, zero=False):
        import torch
        self.dtype, self.nbytes = np.dtype(dtype), int(nbytes)
        guard = -(-max(GUARD, int(row_bytes)) // 256) * 256
        self.start = guard + (align if 0 < align < 16 else 0) + offset_elems * self.dtype.itemsize
        total = -(-(self.start + self.nbytes + guard) // 16) * 16
        pat = sentinel_bytes(dtype)
        self.host = pat[(np.arange(total) - self.start) % len(pat)].copy()
        self.zero = zero
        if zero:
            self.host[self.start:self.start + self.nbytes] = 0
        self.dev = torch.from_numpy(self.host.copy()).to(gpu)
        assert self.dev.data_ptr() % 256 == 0
        addr = self.dev.data_ptr() + self.start
        assert addr % max(align, self.dtype.itemsize) == 0
        assert align >= 16 or addr % 16 != 0, "the pointer was to break 16-byte alignment"
        self.ptr = ctypes.c_void_p(addr)

    def interior(self):
        """The device tensor of the bytes inside the guards."""
        return self.dev[self.start:self.start + self.nbytes]

    def rezero(self):
        self.interior().zero_()

    def read(self, shape):
        """(front guard, the array, back guard) as they are on the device now."""
        raw = self.dev.cpu().numpy()
        body = raw[self.start:self.start + self.nbytes].copy().view(self.dtype).reshape(shape)
        return raw[:self.start], body, raw[self.start + self.nbytes:]

    def guards_hold(self, raw_front, raw_back):
        return (np.array_equal(raw_front, self.host[:self.start]) and
                np.array_equal(raw_back, self.host[self.start + self.nbytes:]))


class Placed:
    """A built case in device memory: inputs in tensors of their own, outputs and scratch in guarded regions."""

    def __init__(self, gpu, built, input_values=None):
        self.built = built
        self.inputs = self.upload(gpu, input_values if input_values is not None else built.inputs)
        self.outputs = {k: Region(gpu, o.nbytes, o.dtype, o.align, o.offset_elems, o.row_bytes, o.zero_on_entry)
                        for k, o in built.outputs.items()}
        self.scratch = {k: Region(gpu, n, np.uint8, align) for k, (n, align) in built.scratch.items()}
        self.ptrs = {k: ctypes.c_void_p(t.data_ptr()) for k, t in self.inputs.items()}
        self.ptrs.update({k: r.ptr for k, r in self.outputs.items()})
        self.ptrs.update({k: r.ptr for k, r in self.scratch.items()})

    @staticmethod
    def upload(gpu, values):
        """name -> uint8 device tensor of the array's bytes (16 zero bytes for an empty one)."""
        import torch
        out = {}
        for k, a in values.items():
            a = np.ascontiguousarray(a)
            out[k] = torch.from_numpy(a.reshape(-1).view(np.uint8).copy() if a.size else np.zeros(16, np.uint8)).to(gpu)
            assert out[k].data_ptr() % 256 == 0
        return out

    def call(self, L, handle, stream):
        self.built.call(L, handle, stream, self.ptrs)

    def read_inputs(self):
        out = {}
        for k, a in self.built.inputs.items():
            raw = self.inputs[k].cpu().numpy()
            out[k] = raw[:a.nbytes].copy().view(a.dtype).reshape(a.shape)
        return out

    def read_outputs(self):
        """name -> (front guard, array, back guard), scratch included (as bytes)."""
        out = {k: r.read(self.built.outputs[k].shape) for k, r in self.outputs.items()}
        out.update({k: r.read((r.nbytes,)) for k, r in self.scratch.items()})
        return out
