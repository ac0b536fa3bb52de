"""The launching entry points of include/train/pp_convt_train.h under the two ABI checks of the data-path entry
points, by their own code, as tests/test_gpu_train_s2_contract.py runs the stride-2 convs':

  tests/test_gpu_abi_guard_bands.py   a call writes only what the header says it writes: every output and the
      workspace lie between guard bands, every float input between two bands of the NaN sentinel (``guard_inputs``),
      so a read past either end that reaches an output makes it NaN and fails the gate; the inputs and their bands
      keep their bits.
  tests/test_gpu_abi_stream_order.py  every launch goes to the stream the call was given.

The cases are in tests/train_up_contract_cases.py: two each for the stride-4 forward and the stride-4 conv, one per
stride for the weight gradient."""
import pytest

import test_gpu_abi_guard_bands as GB
import test_gpu_abi_stream_order as SO
import train_up_contract_cases as TC

pytestmark = pytest.mark.gpu

side = SO.side      # the module-scoped fixture: (stream, a context of its own, spin cycles per millisecond)


@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: c.id)
def test_writes_only_what_the_header_says(gpu, oracle, case):
    GB.test_writes_only_what_the_header_says(gpu, oracle, case, guard_inputs=True)


@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: c.id)
def test_every_step_runs_on_the_given_stream(gpu, oracle, side, case):
    SO.test_every_step_runs_on_the_given_stream(gpu, oracle, side, case)
