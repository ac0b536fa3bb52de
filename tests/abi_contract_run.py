"""Device-side plumbing shared by tests/test_gpu_abi_guard_bands.py and tests/test_gpu_abi_stream_order.py: puts the
arrays of a case of tests/abi_contract_cases.py into device memory the way the header allows a caller to, every
output and scratch buffer between two guard bands of a sentinel bit pattern -- and, on request, every float input
between two bands of the NaN sentinel, so that a read past either end that reaches an output turns it NaN."""
import ctypes

import numpy as np

GUARD = 4096          # bytes on either side, at least; at least one innermost row of the output
INPUT_GUARD = 1 << 16  # bytes of NaN sentinel on either side of a guarded float input: more than a row plus a tile of
#                        pixels of any conv case's activations (at most (35 + 32) pixels x 128 channels x 4 bytes)
# a quiet NaN with a payload for the float types, 0x5A bytes for the integers: neither is a value any case expects
SENTINEL = {np.dtype(np.float16): np.array([0x7E5A], np.uint16).view(np.float16)[0],
            np.dtype(np.float32): np.array([0x7FE5A5A5], np.uint32).view(np.float32)[0],
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

    def __init__(self, gpu, nbytes, dtype, align, offset_elems=0, row_bytes=0, zero=False, guard_bytes=0):
        import torch
        self.dtype, self.nbytes = np.dtype(dtype), int(nbytes)
        guard = -(-max(GUARD, int(row_bytes), int(guard_bytes)) // 256) * 256
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
    """A built case in device memory: inputs in tensors of their own, outputs and scratch in guarded regions.
    ``guard_inputs``: every float input lies between two bands of INPUT_GUARD bytes of its type's NaN sentinel
    (``inputs[k]`` is then the view of the array's bytes inside ``input_buffers[k]``)."""

    def __init__(self, gpu, built, input_values=None, guard_inputs=False):
        self.built = built
        self.input_buffers = {}
        self.inputs = self.upload(gpu, input_values if input_values is not None else built.inputs,
                                  self.input_buffers if guard_inputs else None)
        self.outputs = {k: Region(gpu, o.nbytes, o.dtype, o.align, o.offset_elems, o.row_bytes, o.zero_on_entry,
                                  getattr(o, "guard_bytes", 0)) for k, o in built.outputs.items()}
        self.scratch = {k: Region(gpu, n, np.uint8, align) for k, (n, align) in built.scratch.items()}
        self.ptrs = {k: ctypes.c_void_p(t.data_ptr()) for k, t in self.inputs.items()}
        self.ptrs.update({k: r.ptr for k, r in self.outputs.items()})
        self.ptrs.update({k: r.ptr for k, r in self.scratch.items()})

    @staticmethod
    def upload(gpu, values, buffers=None):
        """name -> uint8 device tensor of the array's bytes (16 zero bytes for an empty one).  With ``buffers`` (a
        dict, filled here) a non-empty float array is uploaded inside a buffer of its type's NaN sentinel, INPUT_GUARD
        bytes on either side; ``buffers[name]`` is (the whole device buffer, its host image)."""
        import torch
        out = {}
        for k, a in values.items():
            a = np.ascontiguousarray(a)
            raw = a.reshape(-1).view(np.uint8).copy() if a.size else np.zeros(16, np.uint8)
            if buffers is not None and a.size and a.dtype in SENTINEL:
                pat = sentinel_bytes(a.dtype)
                host = pat[np.arange(2 * INPUT_GUARD + len(raw)) % len(pat)].copy()     # INPUT_GUARD % len(pat) == 0
                host[INPUT_GUARD:INPUT_GUARD + len(raw)] = raw
                whole = torch.from_numpy(host.copy()).to(gpu)
                buffers[k] = (whole, host)
                out[k] = whole[INPUT_GUARD:INPUT_GUARD + len(raw)]
            else:
                out[k] = torch.from_numpy(raw).to(gpu)
            assert out[k].data_ptr() % 256 == 0
        return out

    def broken_input_guards(self):
        """Names of the guarded inputs whose sentinel bands no longer hold their bits."""
        bad = []
        for k, (whole, host) in self.input_buffers.items():
            now = whole.cpu().numpy()
            n = len(now) - 2 * INPUT_GUARD
            if not (np.array_equal(now[:INPUT_GUARD], host[:INPUT_GUARD]) and
                    np.array_equal(now[INPUT_GUARD + n:], host[INPUT_GUARD + n:])):
                bad.append(k)
        return bad

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
