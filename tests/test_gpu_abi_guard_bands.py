"""Does a device entry point write only what include/pp_hip.h says it writes?

Every data-path case of tests/abi_contract_cases.py, the fused loss and the sparse stem, straight through the C ABI:

  * every output lies inside a larger buffer of a sentinel bit pattern (a NaN payload for float types, 0x5A bytes for
    integers), at least 4 KiB and at least one innermost row on either side, and is itself pre-filled with the
    sentinel -- except a canvas the header wants zero on entry, which holds zeros between sentinel guards;
  * the pointer has the alignment the header demands and no more: where it demands none, 16-byte alignment is broken
    (the targets start 1 and 3 floats into their buffers, the rest at the natural alignment of their type);
  * a caller-sized scratch (pp_loss_workspace_bytes, the stem's documented minimum) is exactly that many bytes, with
    guards.

After the call and a synchronise both guards of every output and scratch hold their bits, every element the header
documents as written equals the reference at the parity test's criterion and no longer holds the sentinel, every
element it documents as not written still does, and every input holds its original bits (pp_paste_batch_dev's in/out
g_centers_dev is compared with the restatement).  A second call into the same buffers, without refilling them, gives
the same bits: the call does not depend on stale contents.  (Before it, a zero-on-entry canvas is zeroed again and an
in/out input restored -- the header's own preconditions.)

The network-side entry points have sentinel-filled destinations in tests/test_gpu_epilogue_abi.py,
tests/test_gpu_bn_train_abi.py and the head kernel's tests; their cases are in the table for
tests/test_gpu_abi_stream_order.py only.  The conv kernels' channel-slice tests prefill neighbouring CHANNELS of the
same tensor and cannot see a store in front of pixel 0 or behind the last pixel: the conv entry points run under this
module's test in tests/test_gpu_conv_contract.py, on the cases of tests/conv_contract_cases.py, with guards that reach
a row and a tile of pixels and with ``guard_inputs``.

Wall time of the module on an MI355X: 4 s for its 198 cases; the slowest takes 0.4 s."""
import numpy as np
import pytest

import abi_contract_cases as T
from abi_contract_run import Placed, sentinel_bytes
from util import Abi

pytestmark = pytest.mark.gpu


def holds_sentinel(a):
    """Per element: does it still hold the sentinel pattern of its type?"""
    pat = sentinel_bytes(a.dtype)
    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8).reshape(-1, a.dtype.itemsize)
    return (raw == pat[None]).all(axis=1).reshape(a.shape)


def check_guards(placed, state, when):
    for k, (front, _, back) in state.items():
        region = placed.outputs.get(k) or placed.scratch[k]
        assert np.array_equal(front, region.host[:region.start]), f"{when}: wrote in front of {k}"
        assert np.array_equal(back, region.host[region.start + region.nbytes:]), f"{when}: wrote behind {k}"


@pytest.mark.parametrize("case", T.guard_cases(), ids=lambda c: c.id)
def test_writes_only_what_the_header_says(gpu, oracle, case, guard_inputs=False):
    """``guard_inputs`` (tests/test_gpu_conv_contract.py): every float input between two bands of the NaN sentinel."""
    import torch
    A = Abi(gpu)
    built = case.build(False)
    want = built.expected(oracle)
    placed = Placed(gpu, built, guard_inputs=guard_inputs)
    placed.call(A.L, A.h, A.stream)
    torch.cuda.synchronize()
    first = placed.read_outputs()
    check_guards(placed, first, "first call")
    got = {k: first[k][1] for k in built.outputs}
    for k, a in got.items():
        written = built.written.get(k)
        still = holds_sentinel(a)
        if written is None:
            assert not still.any(), f"{k}: {int(still.sum())} elements the header documents as written were not"
        else:
            assert not still[written].any(), f"{k}: elements the header documents as written were not"
            assert still[~written].all(), f"{k}: wrote elements the header documents as not written"
    after = placed.read_inputs()
    for k, a in built.inputs.items():
        if k in built.inout:
            got[k] = after[k]
        else:
            assert np.array_equal(T.bits(after[k]), T.bits(a)), f"the call changed its input {k}"
    built.check(got, want)
    # again, into the same buffers as they are now
    for k, o in built.outputs.items():
        if o.zero_on_entry:
            placed.outputs[k].rezero()
    for k in built.inout:
        placed.inputs[k].copy_(torch.from_numpy(built.inputs[k].reshape(-1).view(np.uint8).copy()))
    placed.call(A.L, A.h, A.stream)
    torch.cuda.synchronize()
    second = placed.read_outputs()
    check_guards(placed, second, "second call")
    assert not placed.broken_input_guards(), f"wrote next to the inputs {placed.broken_input_guards()}"
    for k in built.outputs:
        assert np.array_equal(T.bits(second[k][1]), T.bits(first[k][1])), f"{k}: a second call gave other bits"
    again = placed.read_inputs()
    for k in built.inout:
        assert np.array_equal(T.bits(again[k]), T.bits(after[k])), f"{k}: a second call gave other bits"
