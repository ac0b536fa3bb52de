"""pp_adam_step_dev and pp_adam_pack_dev (include/pp_optim.h) under the two ABI checks of the data-path entry points,
by their own code: tests/test_gpu_abi_guard_bands.py (a call writes only p, m, v, the state record, its workspace and
the flat gradient; the pad floats of the moments, the floats between the parameter tensors and every guard keep their
sentinels; the inputs keep their bits; a second call into the same buffers gives the same bits) and
tests/test_gpu_abi_stream_order.py (a side stream with a context of its own, a warm-up on the decoys, a 20 ms
device-side delay, inconclusive -- failed -- when the event had completed at return).  The cases are in
tests/adam_contract_cases.py.

Wall time of the module on an MI355X: see profiles/r25/NOTES.md."""
import pytest

import adam_contract_cases as AC
import test_gpu_abi_guard_bands as GB
import test_gpu_abi_stream_order as SO

pytestmark = pytest.mark.gpu

side = SO.side      # the module-scoped fixture: (stream, a context of its own, spin cycles per millisecond)


@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c.id)
def test_writes_only_what_the_header_says(gpu, oracle, case):
    GB.test_writes_only_what_the_header_says(gpu, oracle, case)


@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c.id)
def test_every_step_runs_on_the_given_stream(gpu, oracle, side, case):
    SO.test_every_step_runs_on_the_given_stream(gpu, oracle, side, case)
