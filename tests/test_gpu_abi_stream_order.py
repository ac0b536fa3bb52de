"""Does every launch, memset and copy of a device entry point go to the stream it was given?

The header promises "everything runs on ``stream``" and "never synchronise"; the overlapped pipeline, the training step
and graph capture rely on it.  Graph capture proves it for the entry points that are captured somewhere in the suite;
this module proves it for every case of tests/abi_contract_cases.py without capturing anything.

Per case, on a second context and a ``torch.cuda.Stream`` (one context per stream, as the header requires):

  warm-up   one call on that stream with the DECOY inputs (same sizes, same host arguments, other values), then a
            synchronise: the call under test allocates nothing, and the decoys sit in the input buffers.  (Four calls
            for the pipelined voxelizer forms: their batches rotate through four workspace slots, each sized on first
            use, and an allocation may wait for the device -- include/pp_hip.h, pp_voxelize_step_dev.)
  then, on the side stream, in order
    1. a device-side delay (a spinning kernel, no host sleep)
    2. an event
    3. ``copy_`` of the real inputs over the decoys (and zeros into a canvas the header wants zero on entry)
    4. the entry point, with the side stream's handle -- the pipelined voxelizer forms make all four of their calls,
       the drain included, here
  the moment the host call returns the event must NOT have completed: otherwise the run proves nothing and the test
  FAILS as inconclusive.  After a synchronise the outputs must equal the reference of the REAL inputs at the parity
  criterion.  A launch, memset or copy that went to the null stream ran while the delay was still spinning, on the
  decoys or on intermediates nothing had written yet, and the comparison fails (every output of the decoy's reference
  differs from the real one: tests/test_abi_contract_cases.py).

The delay.  On an MI355X the host needs 0.14 ms from recording the event to the return of the slowest case's last
call (pp_voxelize_step_dev: the input copy and four calls; pp_ingest_sweeps_dev with its sixteen input copies takes
0.09 ms, most cases 0.03 .. 0.07 ms; the test prints the figure of every case).  DELAY_MS is 20 ms, more than a hundred
times that: host jitter on a shared machine is large and the delay costs milliseconds.  The spin length is calibrated
once per module with events (2 000 000 cycles of the spin kernel took 0.85 ms).

Wall time of the module on an MI355X: about 6 s for its 212 cases."""
import ctypes
import time

import numpy as np
import pytest

import abi_contract_cases as T
from abi_contract_run import Placed

pytestmark = pytest.mark.gpu

DELAY_MS = 20.0


@pytest.fixture(scope="module")
def side(gpu):
    """(stream, a context of its own, spin cycles per millisecond)."""
    import torch
    from pp_amd import _lib
    stream = torch.cuda.Stream(gpu)
    ctx = _lib.Context(gpu.index)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cycles = 2_000_000
    with torch.cuda.stream(stream):
        torch.cuda._sleep(1000)                 # the spin kernel's code object is loaded before it is timed
        e0.record(stream)
        torch.cuda._sleep(cycles)
        e1.record(stream)
    stream.synchronize()
    ms = e0.elapsed_time(e1)
    assert ms > 0.5, f"the spin kernel does not spin ({ms} ms for {cycles} cycles)"
    print(f"spin: {cycles} cycles = {ms:.3f} ms")
    yield stream, ctx, cycles / ms
    stream.synchronize()
    ctx.close()


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_every_step_runs_on_the_given_stream(gpu, oracle, side, case):
    import torch
    from pp_amd import _lib
    stream, ctx, cycles_per_ms = side
    L = _lib.lib()
    real, decoy = case.build(False), case.build(True)
    want = real.expected(oracle)
    placed = Placed(gpu, real, input_values=decoy.inputs)
    staged = Placed.upload(gpu, real.inputs)
    handle = ctypes.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for _ in range(real.warmups):           # warm-up, on the decoys
            for k, o in real.outputs.items():
                if o.zero_on_entry:
                    placed.outputs[k].rezero()
            placed.call(L, ctx.handle, handle)
    stream.synchronize()
    event = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(DELAY_MS * cycles_per_ms))
        event.record(stream)
        t0 = time.perf_counter()
        for k, o in real.outputs.items():
            if o.zero_on_entry:
                placed.outputs[k].rezero()
        for k, t in placed.inputs.items():
            t.copy_(staged[k], non_blocking=True)
        placed.call(L, ctx.handle, handle)
        pending = not event.query()
        host_ms = 1e3 * (time.perf_counter() - t0)
    print(f"{case.id}: host enqueue {host_ms:.3f} ms, delay {DELAY_MS} ms")
    stream.synchronize()
    assert pending, (f"inconclusive: the delay of {DELAY_MS} ms had finished when the call returned after "
                     f"{host_ms:.3f} ms -- either the call waited for the device or the host stalled")
    got = {k: v[1] for k, v in placed.read_outputs().items() if k in real.outputs}
    after = placed.read_inputs()
    for k, a in real.inputs.items():
        if k in real.inout:
            got[k] = after[k]
        else:
            assert np.array_equal(T.bits(after[k]), T.bits(a)), f"the call changed its input {k}"
    real.check(got, want)
