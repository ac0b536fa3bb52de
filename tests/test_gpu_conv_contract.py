"""The conv entry points of include/pp_conv_split.h and include/pp_conv_train.h, and an edge shape of each older conv
kernel of include/pp_hip.h, under the two ABI checks of the data-path entry points, by their own code:

  tests/test_gpu_abi_guard_bands.py   a call writes only what the header says it writes.  Every conv output lies between
      guard bands of at least one output row plus one workgroup tile's width of pixels, so a store in front of pixel 0
      of sample 0 (the transposed kernels' ox = S*j - 1 + px) or behind the last pixel of the last sample (a partial
      tile's rows oy >= H and columns ox >= W) lands in a band; the slice case keeps its sentinels outside channels
      [64, 192).  Every float input lies between two bands of the NaN sentinel (``guard_inputs``): a read past either
      end that reaches an output makes it NaN and fails the gate; the inputs and their bands keep their bits.
  tests/test_gpu_abi_stream_order.py  every launch goes to the stream it was given: a side stream with a context of its
      own, a warm-up on the decoys, a 20 ms device-side delay, inconclusive -- failed -- when the event had completed
      at return.

The cases are in tests/conv_contract_cases.py; none is stream-only.  The walking cases need more items than the
device has compute units, which is asserted here, not skipped.

Measured on an MI355X (256 compute units), largest err / bound per case, the same under both checks (the kernels are
bit-identical from call to call):
    pp_conv3x3_split_nhwc_dev        0.057 (2x3), 0.044 (9x33 B=2, whole and as a slice), 0.063 (the walk)
    pp_conv3x3_split_bare_nhwc_dev   0.040 (2x3, no scale), 0.049 (9x33 B=2, s = 2^7), 0.059 (the walk, s = 2^7)
    pp_conv3x3_s2_split_nhwc_dev     0.023 (2x2), 0.042 (17x70 B=2)
    pp_convt3x3_split_nhwc_dev       0.32 (1x1 stride 4), 0.071 (9x35 stride 2), 0.29 (5x35 stride 4): at stride 4 the
                                     tapless pixels are the table's constant and what is left is the epilogue's rounding
    pp_conv3x3_f16_nhwc_dev          gate 1 0.049, gate 2 0.13;  pp_conv3x3_s2_f16_nhwc_dev  0.049, 0.075
    pp_convt3x3_f16_nhwc_dev         stride 2: 0.083, 0.20;  stride 4: 0.34, 0.34
    pp_conv3x3_wino_nhwc_dev         passes _check; max err 1.5e-6 against MIOpen's 1.5e-6
    pp_pow2_scale_dev, pp_split_pack_dev   exact
    pp_relu_bn_train_*_nhwc_dev      largest e of any key 2.4e-7 (dbias at (3,121,72)) against the bar of 1e-5
No case was inconclusive under the stream-order check (host enqueue 0.02 .. 0.05 ms against the 20 ms delay); no guard
and no input changed.  Wall time of the module: 5 s for its 50 tests; the slowest, the walking case under the guard
bands, takes 0.25 s (the first test also pays 1.5 s of fixtures)."""
import pytest

import conv_contract_cases as CC
import test_gpu_abi_guard_bands as GB
import test_gpu_abi_stream_order as SO

pytestmark = pytest.mark.gpu

side = SO.side      # the module-scoped fixture: (stream, a context of its own, spin cycles per millisecond)


def _walks_here(gpu, case):
    if case.id in CC.WALKING:
        import torch
        units = torch.cuda.get_device_properties(gpu).multi_processor_count
        items = CC.WALKING[case.id]
        assert items > units, (f"{case.id}: the launch has {items} items and this device {units} compute units, so no "
                               f"workgroup walks from item to item and the case does not test what it is for")


@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.id)
def test_writes_only_what_the_header_says(gpu, oracle, case):
    _walks_here(gpu, case)
    GB.test_writes_only_what_the_header_says(gpu, oracle, case, guard_inputs=True)


@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.id)
def test_every_step_runs_on_the_given_stream(gpu, oracle, side, case):
    _walks_here(gpu, case)
    SO.test_every_step_runs_on_the_given_stream(gpu, oracle, side, case)
