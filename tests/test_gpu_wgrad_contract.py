"""pp_conv3x3_split_wgrad_nhwc_dev (include/train/pp_conv_wgrad.h) under the two ABI checks of the data-path entry
points, by their own code, as tests/test_gpu_conv_contract.py runs the other conv entry points:

  tests/test_gpu_abi_guard_bands.py   a call writes only what the header says it writes: dw and the workspace lie
      between guard bands, every float input (x, dz, dz_scale) between two bands of the NaN sentinel
      (``guard_inputs``), so a read past either end that reaches dw makes it NaN and fails the gate; the inputs and
      their bands keep their bits.
  tests/test_gpu_abi_stream_order.py  both launches go to the stream the call was given.

The cases are in tests/wgrad_contract_cases.py.

Measured on an MI355X, largest err / bound, the same under both checks (the kernel is bit-identical from call to
call):
    64->64@9x33 (no scale)  0.11      64->128@17x40 B=2 (s = 2^7)  0.062
No case was inconclusive under the stream-order check (host enqueue 0.04 .. 0.05 ms against the 20 ms delay); no guard
and no input changed."""
import pytest

import test_gpu_abi_guard_bands as GB
import test_gpu_abi_stream_order as SO
import wgrad_contract_cases as WC

pytestmark = pytest.mark.gpu

side = SO.side      # the module-scoped fixture: (stream, a context of its own, spin cycles per millisecond)


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c.id)
def test_writes_only_what_the_header_says(gpu, oracle, case):
    GB.test_writes_only_what_the_header_says(gpu, oracle, case, guard_inputs=True)


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c.id)
def test_every_step_runs_on_the_given_stream(gpu, oracle, side, case):
    SO.test_every_step_runs_on_the_given_stream(gpu, oracle, side, case)
